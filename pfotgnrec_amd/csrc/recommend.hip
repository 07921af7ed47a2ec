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
//
// Layout of the file.  Three kernels - plain, mean-variance, basket - over one argument block (RecArgs, with RecMvArgs for the
// last two), passed by value.  What they share is written once, above them: the opening (rec_user_fragments, rec_block_table,
// rec_next_pass), stage A (rec_score_tile / rec_score_chunk), the exclusion-length clamp, and for the last two the per-user
// header (RecMvUser), the two halves of the admissible set and the empty-slot tail (rec_mv_*).  Only the rank loops are each
// kernel's own (rec_next_pass hands out the members and leaves the `while (pending)` to the kernel: as the loop's condition it
// cost the plain and the mean-variance kernel 10 to 14 VGPRs and two of them a wave of occupancy).  On the host one
// check per argument block (rec_check_common, rec_check_mv) and one launcher (rec_launch: the NJ dispatch, the LDS attribute,
// the launch and its check) serve the three entries.  Behind the three kernels stands the wide form of the mean-variance one
// (two kernels over a workspace, ranks by sorting: its own comment), which shares the opening, stage A, RecMvUser, the rec_mv_*
// pieces and the host checks with them.  Last, the list form (every user ranks a list of its own, one wavefront per user: its
// own comment) takes the key, rec_better, RecMvUser, rec_mv_stock, the empty-slot tail, the host checks and the launcher from
// here and nothing of stage A: a gathered row is no tile.  The three kernels that compute y from a portfolio and serve a list -
// the bounded mean-variance kernel, the wide score kernel, the list form - each have a WEIGHTED form (a weight per
// holding, port_w, in place of 1 / n_holding): new __global__ shells over the shared bodies, a sibling for the wide score kernel.
#include "common.hpp"
#include "mv_value.hpp"
#include <algorithm>
#include <type_traits>

#define PFO_REC_THREADS 256
#define PFO_REC_TILE 16                       // users per workgroup = rows of the MFMA tile
#define PFO_REC_CHUNK 512                     // candidates whose scores are in LDS at a time (32 KB)
#define PFO_REC_SLOTS (PFO_REC_CHUNK / 64)    // keys per lane and user

namespace {

typedef float rec_f32x4 __attribute__((ext_vector_type(4)));

// What the three kernels share: the arguments of pfo_recommend_topk (include/pfotgn.h) and IC, the candidates a row of LDS holds.
struct RecArgs {
  const float *user_emb, *item_emb;
  const int32_t *user_block, *excl_pos, *excl_len;
  const uint8_t* item_ok;
  int64_t U;
  int I, n_t, D, excl_stride, k, IC;
  int32_t *top_pos, *n_valid;
  float* top_score;
  const int32_t* cand_group;                  // the capped forms alone: [I], < 0 = in no group; at most group_cap picks a group
  int group_cap;
  int held_stride;                            // the _held forms alone: held_group i32[U, held_stride], held_len i32[U] - one group id
  const int32_t *held_group, *held_len;       // per holding of the user (< 0: in no group); a group's count starts from them
};
// The mean-variance side (pfo_recommend_mv_topk) but for its five read-only tables, which the kernels take as __restrict__
// parameters of their own (PFO_REC_MV_TABLES); the three diagnostic outputs are the mv kernel's alone.
struct RecMvArgs {
  int n_days, n_stocks, n_ret, port_stride;
  double gamma, lam;
  double *top_fused, *y_out, *fused_out;
  float* score_out;
};

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

// ---- the opening of every kernel: the user fragments, the tile's block table, the passes
// this lane's pieces of user row r: NJ 16-byte pieces per lane cover a row of D <= 16 * NJ floats (a row beyond U reads the last
// user's: its scores are never selected from)
template <int NJ>
__device__ __forceinline__ void rec_user_fragments(float4 (&uf)[NJ], const float* __restrict__ user_emb, int64_t u0, int64_t U, int D) {
  const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  const float4* up = reinterpret_cast<const float4*>(user_emb + min(u0 + r, U - 1) * D);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int d = 16 * j + 4 * q;
    uf[j] = d < D ? up[d >> 2] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}
// ub[i] = the block user u0 + i is scored against, -1 for a row beyond U: served by no pass.  All threads (a barrier);
// returns the users still to be served, a bit each.
__device__ __forceinline__ unsigned rec_block_table(int* ub, const RecArgs& a, int64_t u0) {
  const int tid = threadIdx.x;
  if (tid < PFO_REC_TILE) {
    const int64_t u = u0 + tid;
    int b = -1;
    if (u < a.U) b = a.user_block ? min(max(a.user_block[u], 0), a.n_t - 1) : 0;
    ub[tid] = b;
  }
  __syncthreads();
  unsigned pending = 0;
#pragma unroll
  for (int i = 0; i < PFO_REC_TILE; ++i) pending |= (ub[i] >= 0 ? 1u : 0u) << i;
  return pending;
}
// One pass per distinct block of the tile: takes the block b of the first pending user and every pending user of that block
// (the members, returned) out of `pending`, which is not 0.  The same for every thread.
__device__ __forceinline__ unsigned rec_next_pass(unsigned& pending, const int* ub, int& b) {
  b = ub[__ffs(pending) - 1];
  unsigned members = 0;
#pragma unroll
  for (int i = 0; i < PFO_REC_TILE; ++i) members |= (((pending >> i) & 1u) && ub[i] == b ? 1u : 0u) << i;
  pending &= ~members;
  return members;
}

// ---- stage A
// One 16 x 16 tile of scores: acc[i] = user row 4 q + i . candidate row `item` (this lane's column), uf the lane's pieces of its
// user row.  The ONE place the accumulation order of a score is written down: every kernel below comes here through
// rec_score_chunk, so they agree to the bit.
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

// The scores of the tile's users against candidates [c0, c0 + n) of `items` into sc[16][ICS], candidate c0 + c in column c.
// The caller's barriers stand around it.
template <int NJ>
__device__ __forceinline__ void rec_score_chunk(const float4 (&uf)[NJ], const float* __restrict__ items, int c0, int n, int I, int D,
                                                float* sc, int ICS) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  const int n_tile = (n + 15) >> 4;
  for (int t = wave; t < n_tile; t += 4) {
    const rec_f32x4 acc = rec_score_tile<NJ>(uf, items, min(c0 + 16 * t + r, I - 1), D, q);   // (a column beyond I repeats the last row; never read back)
    // acc[i] = score(user 4 q + i, candidate c0 + 16 t + r)
#pragma unroll
    for (int i = 0; i < 4; ++i) sc[(4 * q + i) * ICS + 16 * t + r] = acc[i];
  }
}

// how much of user u's exclusion row counts
__device__ __forceinline__ int rec_excl_len(const RecArgs& a, int64_t u) {
  return (a.excl_pos && a.excl_stride > 0) ? min(max(a.excl_len[u], 0), a.excl_stride) : 0;
}

// HELD: how much of user u's held-group row counts
__device__ __forceinline__ int rec_held_len(const RecArgs& a, int64_t u) {
  return (a.held_group && a.held_stride > 0) ? min(max(a.held_len[u], 0), a.held_stride) : 0;
}
// HELD, the mean-variance and the basket kernel: the row of the user being served into LDS hg[held_stride] (all threads; the
// caller's next barrier stands behind it); returns its length.  h_u(g) is then rec_held_count(hg, len, g) - every lane reads
// the same word, a broadcast.
__device__ __forceinline__ int rec_held_row(int* hg, const RecArgs& a, int64_t u) {
  const int len = rec_held_len(a, u);
  for (int p = threadIdx.x; p < len; p += PFO_REC_THREADS) hg[p] = a.held_group[u * a.held_stride + p];
  return len;
}
__device__ __forceinline__ int rec_held_count(const int* hg, int len, int g) {   // (g >= 0: a negative entry matches nothing)
  int h = 0;
  for (int p = 0; p < len; ++p) h += (hg[p] == g);
  return h;
}

// ---- what the mean-variance and the basket kernel share per user
struct RecMvUser {
  bool day_ok;          // no day: nothing of this user's is read
  int plen;             // how much of the portfolio row counts
  const double* dayp;   // the day's [n_stocks][n_ret] returns
  __device__ __forceinline__ RecMvUser(const RecMvArgs& m, const double* __restrict__ returns, const int32_t* __restrict__ day_idx,
                                       const int32_t* __restrict__ port_idx, const int32_t* __restrict__ port_len, int64_t u) {
    const int day = day_idx[u];
    day_ok = day >= 0 && day < m.n_days;
    plen = (day_ok && port_idx && m.port_stride > 0) ? min(max(port_len[u], 0), m.port_stride) : 0;
    dayp = returns + (int64_t)(day_ok ? day : 0) * m.n_stocks * m.n_ret;
  }
};
// The admissible set, first half: the row of candidate c in the day's returns, -1 where c takes no part - item_ok, cand_stock
// or the day outside the tables.  Such a candidate is a NaN in LDS yv[I]: every comparison with it is false, so it takes part
// in no count.
__device__ __forceinline__ int rec_mv_stock(const RecArgs& a, const int32_t* __restrict__ cand_stock, int n_stocks, int c, bool day_ok) {
  if (!day_ok || (a.item_ok && !a.item_ok[c])) return -1;
  const int stock = cand_stock[c];
  return stock >= 0 && stock < n_stocks ? stock : -1;
}
// Second half: the exclusion list of user u scattered over yv[I] as NaN.  All threads; a barrier before and after.
__device__ __forceinline__ void rec_mv_exclude(double* yv, const RecArgs& a, int64_t u) {
  __syncthreads();
  const int len = rec_excl_len(a, u);
  for (int e = threadIdx.x; e < len; e += PFO_REC_THREADS) {
    const int p = a.excl_pos[u * a.excl_stride + e];
    if (p >= 0 && p < a.I) yv[p] = __builtin_nan("");                // (duplicates store the same value)
  }
  __syncthreads();
}

// slots n .. k - 1 of user u's output row are empty: -1 / -inf / -inf; n_valid[u] = n
__device__ __forceinline__ void rec_mv_empty_slots(int32_t* __restrict__ top_pos, float* __restrict__ top_score, double* __restrict__ top_fused,
                                                   int32_t* __restrict__ n_valid, int64_t u, int k, int n) {
  const int tid = threadIdx.x;
  if (tid >= n && tid < k) {                                         // (k <= 64: a thread each)
    top_pos[u * k + tid] = -1;
    top_score[u * k + tid] = -__builtin_inff();
    top_fused[u * k + tid] = -__builtin_inf();
  }
  if (tid == 0 && n_valid) n_valid[u] = n;
}

// the canonical order: is (f, c) before the best so far (bf, bc)?  bc < 0: there is none yet
__device__ __forceinline__ bool rec_better(double f, int c, double bf, int bc) { return bc < 0 || f > bf || (f == bf && c > bc); }

// ---------------------------------------------------------------------------------------------
// CAPPED (pfo_recommend_topk_capped): the walk skips a candidate whose group holds group_cap picks already.  The capped top-k of
// A u B is the capped top-k of (capped top-k of A) u B, so the walk over chunks stays as it is and the counts start from zero in
// every chunk: once a round's winner is known its group is read (a chunk candidate's from LDS grp[IC] beside ok[], a carried
// one's from its owner's lg), the picks of that group in next[] are counted with a ballot, and at the cap every lane clears
// its keys of that group - the chunk's, and the carried list's.
// HELD (pfo_recommend_topk_capped_held): the count of a group starts from h_u(g), the entries of the user's held-group row that
// name it - in every chunk, for a candidate dropped over A has cap - h_u(g) members of its group before it in A, hence in A u B.
// The rows of the tile's 16 users go to LDS once (hg[16][held_stride], an entry that does not count as -1), and beside them
// hc[16][held_stride]: the ids whose h_u has reached the cap already - the groups closed from the start - packed to the front of
// the row, with hn[32]: how much of each hg row counts and how many closed ids each hc row holds.  A user that holds nothing
// costs nothing: when a chunk is loaded a lane clears the admissible bit of its candidates of every closed group (one broadcast
// read per candidate and closed id); in a round the entries that name the winner's group are counted with a ballot per 64
// entries of the row and added to the ballot count of the picks.
template <int NJ, bool CAPPED = false, bool HELD = false>
__global__ __launch_bounds__(PFO_REC_THREADS) void recommend_topk_kernel(const RecArgs a) {
  static_assert(CAPPED || !HELD, "held rows count against a cap");
  const float *__restrict__ user_emb = a.user_emb, *__restrict__ item_emb = a.item_emb;
  const int32_t* __restrict__ excl_pos = a.excl_pos;
  const uint8_t* __restrict__ item_ok = a.item_ok;
  int32_t *__restrict__ top_pos = a.top_pos, *__restrict__ n_valid = a.n_valid;
  float* __restrict__ top_score = a.top_score;
  const int I = a.I, D = a.D, k = a.k, IC = a.IC, excl_stride = a.excl_stride;
  const int ICS = IC + 4;                                            // row stride: the four user rows a half-wave writes fall on different banks
  extern __shared__ float lds[];
  float* sc = lds;                                                    // [16][ICS]
  uint8_t* ok = reinterpret_cast<uint8_t*>(sc + PFO_REC_TILE * ICS);  // [IC]
  int* grp = reinterpret_cast<int*>(ok + IC);                         // [IC], CAPPED: the group of a chunk candidate (IC is a multiple of 16)
  const int HS = HELD ? a.held_stride : 0;
  int* hg = grp + IC;                                                 // [16][HS], HELD: the held-group rows of the tile's users
  int* hc = hg + PFO_REC_TILE * HS;                                   // [16][HS], HELD: the ids of the groups closed from the start, packed
  int* hn = hc + PFO_REC_TILE * HS;                                   // [32], HELD: the length of each hg row, then of each hc row
  __shared__ int ub[PFO_REC_TILE];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t u0 = (int64_t)blockIdx.x * PFO_REC_TILE;

  float4 uf[NJ];
  rec_user_fragments<NJ>(uf, user_emb, u0, a.U, D);
  if constexpr (HELD) {
    if (tid < PFO_REC_TILE) hn[tid] = u0 + tid < a.U ? rec_held_len(a, u0 + tid) : 0;
    __syncthreads();
    for (int e = tid; e < PFO_REC_TILE * HS; e += PFO_REC_THREADS) {  // (HS == 0: no entry, and nothing below divides)
      const int us = e / HS, p = e - us * HS;
      int g = -1;
      if (p < hn[us]) g = a.held_group[(u0 + us) * HS + p];
      hg[e] = g < 0 ? -1 : g;
    }
    __syncthreads();
    for (int e = tid; e < PFO_REC_TILE * HS; e += PFO_REC_THREADS) {
      const int us = e / HS, g = hg[e];
      int cnt = 0;
      if (g >= 0) cnt = rec_held_count(hg + us * HS, hn[us], g);
      hc[e] = cnt >= a.group_cap ? g : -1;                            // (group_cap >= 1: cnt == 0 closes nothing)
    }
    __syncthreads();
    if (tid < PFO_REC_TILE) {                                         // the closed ids to the front of the row (nc <= p: in place)
      int nc = 0;
      for (int p = 0; p < hn[tid]; ++p) {
        const int g = hc[tid * HS + p];
        if (g >= 0) hc[tid * HS + nc++] = g;
      }
      hn[PFO_REC_TILE + tid] = nc;
    }                                                                 // (the block table's barrier stands behind it)
  }
  unsigned pending = rec_block_table(ub, a, u0);
  while (pending) {
    int b;
    const unsigned members = rec_next_pass(pending, ub, b);
    const float* items = item_emb + (int64_t)b * I * D;

    unsigned long long list[4] = {0ull, 0ull, 0ull, 0ull};           // lane t: rank t of user 4 * wave + i so far
    int lg[4] = {-1, -1, -1, -1};                                    // CAPPED: the group of list[i]
    for (int c0 = 0; c0 < I; c0 += IC) {
      const int n = min(IC, I - c0);
      __syncthreads();                                               // the previous chunk's keys have been taken from LDS
      // ---- A: scores of candidates [c0, c0 + n)
      rec_score_chunk<NJ>(uf, items, c0, n, I, D, sc, ICS);
      for (int c = tid; c < n; c += PFO_REC_THREADS) ok[c] = item_ok ? item_ok[c0 + c] : (uint8_t)1;
      if constexpr (CAPPED)
        for (int c = tid; c < n; c += PFO_REC_THREADS) grp[c] = a.cand_group[c0 + c];
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
          const int len = rec_excl_len(a, u);
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
          if constexpr (HELD) {                                      // the groups closed from the start take no part
            const int nc = __builtin_amdgcn_readfirstlane(hn[PFO_REC_TILE + us]);
            if (nc > 0) {
#pragma unroll 1
              for (int m = 0; m < PFO_REC_SLOTS; ++m) {                // (a slot at a time: one group id in a register)
                if (!((adm >> m) & 1u)) continue;
                const int gc = grp[lane + 64 * m];                     // (an admissible bit: lane + 64 m < n)
                for (int p = 0; p < nc; ++p)
                  if (hc[us * HS + p] == gc) adm &= ~(1u << m);        // (the same word for every lane; gc < 0 matches nothing)
              }
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
        int ng[4] = {-1, -1, -1, -1};                                // CAPPED: the group of next[i]
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
            int gw = -1;                                             // CAPPED: the winner's group (the same for every lane)
            if constexpr (CAPPED) {
              const int rel = (int)(uint32_t)(best[i] & 0xffffffffull) - c0;
              if (rel >= 0) gw = grp[rel];                           // (a carried candidate lies before the chunk)
              else gw = __shfl(lg[i], __ffsll((unsigned long long)__ballot(list[i] == best[i])) - 1, 64);
            }
            // positions are distinct, so exactly one key of the wavefront equals the winner: its owner clears it
            if (list[i] == best[i]) list[i] = 0ull;
#pragma unroll
            for (int m = 0; m < PFO_REC_SLOTS; ++m)
              if (key[i][m] == best[i]) key[i][m] = 0ull;
            if (lane == t) next[i] = best[i];
            if constexpr (CAPPED) {
              if (lane == t) ng[i] = gw;
              int h = 0;                                             // HELD: what the user holds of the winner's group
              if constexpr (HELD) {
                if (gw >= 0) {                                       // (the same for every lane)
                  const int len = __builtin_amdgcn_readfirstlane(hn[4 * wave + i]);
                  for (int p0 = 0; p0 < len; p0 += 64) h += __popcll(__ballot(p0 + lane < len && hg[(4 * wave + i) * HS + p0 + lane] == gw));
                }
              }
              if (gw >= 0 && __popcll(__ballot(ng[i] == gw)) + h >= a.group_cap) {   // the group is full: nobody else of it is taken
                if (lg[i] == gw) list[i] = 0ull;
#pragma unroll
                for (int m = 0; m < PFO_REC_SLOTS; ++m)
                  if (key[i][m] != 0ull && grp[lane + 64 * m] == gw) key[i][m] = 0ull;   // (a key: lane + 64 m < n)
              }
            }
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) list[i] = next[i];
        if constexpr (CAPPED) {
#pragma unroll
          for (int i = 0; i < 4; ++i) lg[i] = ng[i];
        }
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
//   A  scores of the tile's 16 users against ALL I <= 2048 candidates of a block, as above (rec_score_chunk), into LDS [16][I].
//   Then the users of the pass one at a time, all four wavefronts on one user:
//   B  y_mv of every candidate in fp64 (pfo_mv_value, the arithmetic mv_select_kernel runs) into LDS y[I]; a candidate that is
//      not admissible - item_ok, cand_stock or the day outside the tables (rec_mv_stock), a NaN y, then the exclusion list
//      (rec_mv_exclude) - is a NaN there: every comparison with it is false, so it takes part in no count below.
//   C  average-tie ranks of y and of the fp32 score by counting over LDS (scipy's rankdata is less + (equal + 1) / 2), blended
//      into `fused` in registers (a thread owns candidates tid, tid + 256, ...: eight at most); after a barrier fused replaces y.
//   D  the place of a candidate in the canonical order (fused descending, the larger position first among equal values) is
//      the number of candidates before it, by counting again; places below k write the output row.
// LDS: 8 I (y / fused) + 16 (I + 4) 4 (scores) bytes, 144 KB at I = 2048 of the 160 KB a workgroup may take - one workgroup per
// CU there, four at I = 500.  About 3 I^2 comparisons per user.
#define PFO_RMV_PER_THREAD (PFO_RECOMMEND_MV_MAX_ITEMS / PFO_REC_THREADS)

// cand_stock, returns, day_idx, port_idx and port_len stay __restrict__ kernel parameters: a qualifier on a struct member or
// a local tells the compiler nothing, and without it what all lanes read alike - the holdings, their return rows, the day -
// is no longer read with scalar loads (the two kernels then ran 3.4 % and 1.2 % longer).
#define PFO_REC_MV_TABLES                                                                                     \
  const int32_t *__restrict__ cand_stock, const double *__restrict__ returns, const int32_t *__restrict__ day_idx, \
      const int32_t *__restrict__ port_idx, const int32_t *__restrict__ port_len
// CAPPED (pfo_recommend_mv_topk_capped): a candidate survives iff fewer than group_cap admissible candidates of its own group
// stand before it in the canonical order, and the capped list is the first k survivors.  So one more counting pass between C
// and D, over fused and the group ids in LDS (grp[IC] behind the scores, 4 I bytes more: 152 KB at I = 2048): a candidate at
// or beyond the cap becomes a NaN in LDS and in its owner's register, and D runs over the survivors as it is.  The diagnostics
// keep the uncapped values.  About I^2 comparisons more per user, four candidates per LDS read (fused and grp are NaN / -1
// from I up to the next multiple of 16, and the dynamic part starts 16-byte aligned here).
// HELD (pfo_recommend_mv_topk_capped_held): the count form with a start - a candidate survives iff the same-group candidates
// before it plus h_u(g) stay below the cap.  The row of the user being ranked lies in LDS behind grp (hg[held_stride], at most
// 1 KB: 156 928 bytes at I = 2048); a thread counts h for each candidate of its own and, where that alone reaches the cap - a
// group closed from the start - skips the counting pass for it.
// WEIGHTED (pfo_recommend_mv_topk_weighted): y is pfo_mv_value_weighted over the user's row of port_w f64[U, port_stride]
// beside port_idx - one more __restrict__ kernel parameter, for the reason given above the table macro.  Nothing else changes, and
// the unweighted instantiations never see the parameter (their kernels do not have it).
template <int NJ, bool CAPPED, bool HELD = false, bool WEIGHTED = false>
__device__ __forceinline__ void recommend_mv_topk_body(const RecArgs& a, const RecMvArgs& m, PFO_REC_MV_TABLES,
                                                       const double* __restrict__ port_w = nullptr) {
  static_assert(CAPPED || !HELD, "held rows count against a cap");
  static_assert(!WEIGHTED || !CAPPED, "the capped forms take no weights");
  const float *__restrict__ user_emb = a.user_emb, *__restrict__ item_emb = a.item_emb;
  int32_t* __restrict__ top_pos = a.top_pos;
  float *__restrict__ top_score = a.top_score, *__restrict__ score_out = m.score_out;
  double *__restrict__ top_fused = m.top_fused, *__restrict__ y_out = m.y_out, *__restrict__ fused_out = m.fused_out;
  const int I = a.I, D = a.D, k = a.k, IC = a.IC;
  const double lam = m.lam;
  const int ICS = IC + 4;
  extern __shared__ double lds_mv[];
  double* yv = lds_mv;                                               // [IC]: y, then fused, of the user being ranked
  if constexpr (CAPPED) {                                            // (16-byte aligned for the cap pass's wide reads)
    extern __shared__ __attribute__((aligned(16))) double lds_mv_capped[];
    yv = lds_mv_capped;
  }
  float* sc = reinterpret_cast<float*>(yv + IC);                     // [16][ICS]
  int* grp = reinterpret_cast<int*>(sc + PFO_REC_TILE * ICS);        // [IC], CAPPED: the group of every candidate
  int* hg = grp + IC;                                                // [held_stride], HELD: the held-group row of the user being ranked
  __shared__ int ub[PFO_REC_TILE];
  __shared__ int n_adm;
  const int tid = threadIdx.x;
  const int64_t u0 = (int64_t)blockIdx.x * PFO_REC_TILE;
  const double nan = __builtin_nan("");

  float4 uf[NJ];
  rec_user_fragments<NJ>(uf, user_emb, u0, a.U, D);
  if constexpr (CAPPED) {
    // (the block table's barrier stands behind it; from I up to the next multiple of 16 a NaN that nobody overwrites: the cap
    // pass reads four candidates at a time)
    for (int c = tid; c < IC; c += PFO_REC_THREADS) grp[c] = c < I ? a.cand_group[c] : -1;
    for (int c = I + tid; c < IC; c += PFO_REC_THREADS) yv[c] = nan;
  }
  unsigned pending = rec_block_table(ub, a, u0);
  while (pending) {
    int b;
    const unsigned members = rec_next_pass(pending, ub, b);
    // ---- A: scores of all candidates (the previous pass ended on a barrier)
    rec_score_chunk<NJ>(uf, item_emb + (int64_t)b * I * D, 0, I, I, D, sc, ICS);
    __syncthreads();

    for (int us = 0; us < PFO_REC_TILE; ++us) {
      if (!((members >> us) & 1u)) continue;                         // (the same for every thread)
      const int64_t u = u0 + us;
      const float* su = sc + us * ICS;
      if (tid == 0) n_adm = 0;
      int hlen = 0;                                                  // HELD: how much of hg counts (rec_mv_exclude's barriers stand behind the row)
      if constexpr (HELD) hlen = rec_held_row(hg, a, u);
      // ---- B: y_mv, NaN where the candidate is not admissible
      const RecMvUser h(m, returns, day_idx, port_idx, port_len, u);
      for (int c = tid; c < I; c += PFO_REC_THREADS) {
        if (score_out) score_out[u * I + c] = su[c];
        const int stock = rec_mv_stock(a, cand_stock, m.n_stocks, c, h.day_ok);
        if constexpr (WEIGHTED)
          yv[c] = stock < 0 ? nan
                            : pfo_mv_value_weighted(h.dayp, stock, m.n_stocks, m.n_ret, port_idx + u * m.port_stride,
                                                    port_w + u * m.port_stride, h.plen, m.gamma);
        else
          yv[c] = stock < 0 ? nan : pfo_mv_value<true>(h.dayp, stock, m.n_stocks, m.n_ret, port_idx + u * m.port_stride, h.plen, m.gamma);
      }
      rec_mv_exclude(yv, a, u);
      // ---- C: ranks over the admissible candidates, blended
      double fused[PFO_RMV_PER_THREAD];
      int mine = 0;
#pragma unroll
      for (int s = 0; s < PFO_RMV_PER_THREAD; ++s) fused[s] = nan;
#pragma unroll
      for (int s = 0; s < PFO_RMV_PER_THREAD; ++s) {
        const int c = tid + PFO_REC_THREADS * s;
        if (PFO_REC_THREADS * s >= I) break;
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
        fused[s] = pfo_mv_blend(pfo_mv_avg_rank(ly, ey), pfo_mv_avg_rank(ls, es), lam);   // main.py:282-286
        ++mine;
      }
      __syncthreads();                                               // every y has been read
#pragma unroll
      for (int s = 0; s < PFO_RMV_PER_THREAD; ++s) {
        const int c = tid + PFO_REC_THREADS * s;
        if (c < I) {
          yv[c] = fused[s];
          if (fused_out) fused_out[u * I + c] = fused[s];
        }
      }
      if constexpr (!CAPPED)
        if (mine) atomicAdd(&n_adm, mine);
      __syncthreads();
      if constexpr (CAPPED) {
        // ---- the cap: the same-group candidates before this one in the canonical order, counted
        unsigned full = 0;                                           // bit s: candidate tid + 256 s finds its group full
#pragma unroll
        for (int s = 0; s < PFO_RMV_PER_THREAD; ++s) {
          const int c = tid + PFO_REC_THREADS * s;
          if (PFO_REC_THREADS * s >= I) break;
          const double fi = fused[s];
          if (c >= I || !(fi == fi)) continue;
          const int g = grp[c];
          if (g < 0) continue;
          int before = 0;
          if constexpr (HELD) {                                      // the count starts from what the user holds of the group
            before = rec_held_count(hg, hlen, g);
            if (before >= a.group_cap) {                             // closed from the start
              full |= 1u << s;
              continue;
            }
          }
          const double2* f2 = reinterpret_cast<const double2*>(yv);
          const int4* g4 = reinterpret_cast<const int4*>(grp);
#pragma unroll 2
          for (int j = 0; j < IC; j += 4) {                          // (every comparison with a NaN is false)
            const double2 fa = f2[j >> 1], fb = f2[(j >> 1) + 1];
            const int4 gj = g4[j >> 2];
            before += ((gj.x == g) & ((fa.x > fi) | ((fa.x == fi) & (j > c)))) + ((gj.y == g) & ((fa.y > fi) | ((fa.y == fi) & (j + 1 > c)))) +
                      ((gj.z == g) & ((fb.x > fi) | ((fb.x == fi) & (j + 2 > c)))) + ((gj.w == g) & ((fb.y > fi) | ((fb.y == fi) & (j + 3 > c))));
          }
          if (before >= a.group_cap) full |= 1u << s;
        }
        __syncthreads();                                             // every fused has been read
#pragma unroll
        for (int s = 0; s < PFO_RMV_PER_THREAD; ++s) {
          if (!((full >> s) & 1u)) continue;
          yv[tid + PFO_REC_THREADS * s] = nan;
          fused[s] = nan;
          --mine;
        }
        if (mine) atomicAdd(&n_adm, mine);
        __syncthreads();
      }
      // ---- D: the first k of the canonical order
#pragma unroll
      for (int s = 0; s < PFO_RMV_PER_THREAD; ++s) {
        const int c = tid + PFO_REC_THREADS * s;
        if (PFO_REC_THREADS * s >= I) break;
        const double fi = fused[s];
        if (c >= I || !(fi == fi)) continue;
        int before = 0;
        for (int j = 0; j < I; ++j) {
          const double fj = yv[j];
          before += (fj > fi) || (fj == fi && j > c);
        }
        if (before < k) {
          const float sv = su[c];
          top_pos[u * k + before] = c;
          top_score[u * k + before] = sv == 0.f ? 0.f : sv;          // a zero score is handed out as +0
          top_fused[u * k + before] = fi;
        }
      }
      rec_mv_empty_slots(top_pos, top_score, top_fused, a.n_valid, u, k, min(k, n_adm));
      __syncthreads();                                               // n_adm and y are free for the next user
    }
  }
}

// (the body inlined into its kernel, not the kernel itself: written as the kernel, the D <= 176 instantiation takes 165 VGPRs
// instead of 163 and loses its third wave per SIMD)
template <int NJ, bool CAPPED = false, bool HELD = false>
__global__ __launch_bounds__(PFO_REC_THREADS) void recommend_mv_topk_kernel(const RecArgs a, const RecMvArgs m, PFO_REC_MV_TABLES) {
  recommend_mv_topk_body<NJ, CAPPED, HELD>(a, m, cand_stock, returns, day_idx, port_idx, port_len);
}
template <int NJ>
__global__ __launch_bounds__(PFO_REC_THREADS) void recommend_mv_topk_weighted_kernel(const RecArgs a, const RecMvArgs m, PFO_REC_MV_TABLES,
                                                                                     const double* __restrict__ port_w) {
  recommend_mv_topk_body<NJ, false, false, true>(a, m, cand_stock, returns, day_idx, port_idx, port_len, port_w);
}

// ---------------------------------------------------------------------------------------------
// Basket top-k: the list of recommend_mv_topk_kernel taken one pick at a time, each pick joining the holdings before the next
// is ranked (include/pfotgn.h states the rounds).  Same launch shape and the same stage A.  Per user, all four wavefronts:
//   B  the admissible set once (rec_mv_stock, rec_mv_exclude over LDS y[I]) - read back into a bit per owned candidate (a
//      thread owns candidates tid, tid + 256, ...); mu, var and the covariance sum over the portfolio of every owned candidate
//      in registers (pfo_mv_mean / pfo_mv_var / pfo_mv_add_cov: pfo_mv_value's pieces).
//   k rounds of
//   C  y of the round from the three registers (pfo_mv_finish) into LDS y[I], NaN where the candidate takes no part, and NaN
//      over its score in the user's LDS row likewise (the owner keeps the score in a register; the row is this user's alone):
//      the two rank counts of stage C above then need no mask, and run over four candidates per LDS read (y and the row are
//      NaN from I up to the next multiple of 16); the blend as above;
//   P  the pick: the arg-max of (fused, position) (rec_better) over the thread's candidates, the wavefront (shuffles), the
//      workgroup (four LDS slots).  Its owner writes slot r of the output row, clears its bit and sets y[pick] to NaN; every
//      thread adds the pick's covariance to its candidates' sums - one n_ret-long pass per candidate and round, nothing else
//      is recomputed.
// LDS as above (the per-candidate values are registers; the dynamic part starts 16-byte aligned for the wide reads).
// 2 k I^2 comparisons and (held + k - 1) I n_ret multiply-adds per user.
// Two barriers per round; every loop bound between them depends on k, I and the pick (the same for all threads) alone.
// CAPPED (pfo_recommend_basket_topk_capped): a group that holds group_cap picks leaves the pool.  After a pick every thread
// reads the pick's group from LDS (grp[IC] behind the scores - no group id lives in a register across a round), counts it among
// the earlier picks' groups (pick_g[], k ints of LDS: slot r is written in round r and read from round r + 1 on, two barriers
// later) and, once the group is full, takes its own candidates of that group out: the alive bit, NaN in y and in the score row.
// HELD (pfo_recommend_basket_topk_capped_held): the row of the user being served lies in LDS behind grp (hg[held_stride], as in
// the mean-variance kernel).  In B the owner of a candidate counts h_u of its group and keeps a candidate of a group closed from
// the start out of the pool - no alive bit, NaN in y and in the score row, so it takes part in no rank count of round 0 either;
// after a pick every thread starts the pick's count from h_u(gw), one broadcast read per entry of the row.
template <int NJ, bool CAPPED = false, bool HELD = false>
__global__ __launch_bounds__(PFO_REC_THREADS) void recommend_basket_topk_kernel(const RecArgs a, const RecMvArgs m, PFO_REC_MV_TABLES) {
  static_assert(CAPPED || !HELD, "held rows count against a cap");
  const float *__restrict__ user_emb = a.user_emb, *__restrict__ item_emb = a.item_emb;
  int32_t* __restrict__ top_pos = a.top_pos;
  float* __restrict__ top_score = a.top_score;
  double* __restrict__ top_fused = m.top_fused;
  const int I = a.I, D = a.D, k = a.k, IC = a.IC, n_stocks = m.n_stocks, n_ret = m.n_ret;
  const double gamma = m.gamma, lam = m.lam;
  const int ICS = IC + 4;
  extern __shared__ __attribute__((aligned(16))) double lds_basket[];
  double* yv = lds_basket;                                           // [IC]: y of the round, NaN = takes no part
  float* sc = reinterpret_cast<float*>(yv + IC);                     // [16][ICS]
  __shared__ int ub[PFO_REC_TILE];
  __shared__ double wave_f[PFO_REC_THREADS / 64];                    // the best (fused, position) of each wavefront
  __shared__ int wave_c[PFO_REC_THREADS / 64];
  int* grp = reinterpret_cast<int*>(sc + PFO_REC_TILE * ICS);        // [IC], CAPPED: the group of every candidate
  __shared__ int pick_g[CAPPED ? 64 : 1];                            // CAPPED: the group of pick r of the user being served
  int* hg = grp + IC;                                                // [held_stride], HELD: the held-group row of the user being served
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t u0 = (int64_t)blockIdx.x * PFO_REC_TILE;
  const double nan = __builtin_nan("");
  const double inv = pfo_mv_inv(n_ret);

  float4 uf[NJ];
  rec_user_fragments<NJ>(uf, user_emb, u0, a.U, D);
  if constexpr (CAPPED)
    for (int c = tid; c < I; c += PFO_REC_THREADS) grp[c] = a.cand_group[c];   // (the block table's barrier stands behind it)
  unsigned pending = rec_block_table(ub, a, u0);
  while (pending) {
    int b;
    const unsigned members = rec_next_pass(pending, ub, b);
    // ---- A: scores of all candidates (the previous pass ended on a barrier)
    rec_score_chunk<NJ>(uf, item_emb + (int64_t)b * I * D, 0, I, I, D, sc, ICS);
    __syncthreads();

    for (int us = 0; us < PFO_REC_TILE; ++us) {
      if (!((members >> us) & 1u)) continue;                         // (the same for every thread)
      const int64_t u = u0 + us;
      float* su = sc + us * ICS;                                     // the user's scores; NaN where the candidate takes no part
      const RecMvUser h(m, returns, day_idx, port_idx, port_len, u);
      const double* dayp = h.dayp;
      int hlen = 0;                                                  // HELD: how much of hg counts (rec_mv_exclude's barriers stand behind the row)
      if constexpr (HELD) hlen = rec_held_row(hg, a, u);
      // ---- B: the admissible set, then mu, var and the covariance sum over the portfolio
      for (int c = tid; c < IC; c += PFO_REC_THREADS) yv[c] = c < I && rec_mv_stock(a, cand_stock, m.n_stocks, c, h.day_ok) >= 0 ? 0.0 : nan;
      rec_mv_exclude(yv, a, u);
      double mu[PFO_RMV_PER_THREAD], var[PFO_RMV_PER_THREAD], ssum[PFO_RMV_PER_THREAD];
      float score[PFO_RMV_PER_THREAD];
      unsigned alive = 0;                                            // bit s: candidate tid + 256 s is in the pool
#pragma unroll
      for (int s = 0; s < PFO_RMV_PER_THREAD; ++s) {
        const int c = tid + PFO_REC_THREADS * s;
        mu[s] = var[s] = ssum[s] = 0.0;
        score[s] = 0.f;
        if constexpr (HELD) {                                        // a group closed from the start is not in the pool of round 0
          if (c < I && yv[c] == yv[c]) {
            const int g = grp[c];
            if (g >= 0 && rec_held_count(hg, hlen, g) >= a.group_cap) yv[c] = nan;   // (the owner's slot: nobody else reads it here)
          }
        }
        if (c < I && yv[c] == yv[c]) {
          alive |= 1u << s;
          score[s] = su[c];
          const double* ri = dayp + (int64_t)cand_stock[c] * n_ret;
          mu[s] = pfo_mv_mean(ri, n_ret);
          var[s] = pfo_mv_var(ri, mu[s], n_ret, inv);
        } else if (c < IC) {
          su[c] = __builtin_nanf("");
        }
      }
      // one more holding: row st of the day (in range) joins every pooled candidate's sum
      auto hold = [&](int st) {
        const double* rp = dayp + (int64_t)st * n_ret;
        const double mp = pfo_mv_mean(rp, n_ret);
#pragma unroll
        for (int s = 0; s < PFO_RMV_PER_THREAD; ++s) {
          if (!((alive >> s) & 1u)) continue;
          const double* ri = dayp + (int64_t)cand_stock[tid + PFO_REC_THREADS * s] * n_ret;
          ssum[s] = pfo_mv_add_cov(ssum[s], ri, mu[s], rp, mp, n_ret, inv);
        }
      };
      int n_hold = 0;
      for (int p = 0; p < h.plen; ++p) {
        const int st = port_idx[u * m.port_stride + p];
        if ((unsigned)st >= (unsigned)n_stocks) continue;
        ++n_hold;
        hold(st);
      }

      int n_pick = 0;
      for (int rd = 0; rd < k; ++rd) {
        // ---- C: y of this round (the slot of a candidate outside the pool is NaN already), ranks, blend
        double yr[PFO_RMV_PER_THREAD];
#pragma unroll
        for (int s = 0; s < PFO_RMV_PER_THREAD; ++s) {
          yr[s] = nan;
          if (!((alive >> s) & 1u)) continue;
          const int c = tid + PFO_REC_THREADS * s;
          yr[s] = pfo_mv_finish(mu[s], gamma, var[s], ssum[s], n_hold);
          yv[c] = yr[s];
          su[c] = yr[s] == yr[s] ? score[s] : __builtin_nanf("");
        }
        __syncthreads();
        double bf = 0.0;
        int bc = -1;                                                 // the best (fused, position) so far, -1: none
#pragma unroll
        for (int s = 0; s < PFO_RMV_PER_THREAD; ++s) {
          const int c = tid + PFO_REC_THREADS * s;
          const double yi = yr[s];
          if (!(yi == yi)) continue;                                 // outside the pool, or a NaN y: out of this round only
          const float si = score[s];
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
          if (f == f && rec_better(f, c, bf, bc)) {
            bf = f;
            bc = c;
          }
        }
        // ---- P: the first of the canonical order
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
          const double of = __shfl_xor(bf, off, 64);
          const int oc = __shfl_xor(bc, off, 64);
          if (oc >= 0 && rec_better(of, oc, bf, bc)) {
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
          if (oc >= 0 && rec_better(of, oc, bf, bc)) {
            bf = of;
            bc = oc;
          }
        }
        if (bc < 0) break;                                           // nobody took part (the same for every thread): the list ends
        if (tid == (bc & (PFO_REC_THREADS - 1))) {
          alive &= ~(1u << (bc / PFO_REC_THREADS));
          yv[bc] = nan;
          const float sv = su[bc];
          su[bc] = __builtin_nanf("");
          top_pos[u * k + rd] = bc;
          top_score[u * k + rd] = sv == 0.f ? 0.f : sv;              // a zero score is handed out as +0
          top_fused[u * k + rd] = bf;
        }
        if constexpr (CAPPED) {
          const int gw = grp[bc];                                    // (the same for every thread)
          if (tid == 0) pick_g[rd] = gw;
          if (gw >= 0) {
            int held = 1;
            if constexpr (HELD) held += rec_held_count(hg, hlen, gw);
            for (int r = 0; r < rd; ++r) held += (pick_g[r] == gw);
            if (held >= a.group_cap) {                               // the group is full: it leaves the pool
#pragma unroll
              for (int s = 0; s < PFO_RMV_PER_THREAD; ++s) {
                const int c = tid + PFO_REC_THREADS * s;
                if (((alive >> s) & 1u) && grp[c] == gw) {
                  alive &= ~(1u << s);
                  yv[c] = nan;
                  su[c] = __builtin_nanf("");
                }
              }
            }
          }
        }
        ++n_pick;
        if (rd + 1 < k) {
          ++n_hold;
          hold(cand_stock[bc]);                                      // (in range: the pick was in the pool)
        }
      }
      rec_mv_empty_slots(top_pos, top_score, top_fused, a.n_valid, u, k, n_pick);
      __syncthreads();                                               // y and the wavefront slots are free for the next user
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The wide form of the portfolio-aware top-k: recommend_mv_topk_kernel's contract for lists LDS cannot hold (I up to
// PFO_RECOMMEND_MV_WIDE_MAX_ITEMS), its state in a caller-owned workspace and its ranks found by sorting.  Two launches per slab of
// users (the host cuts U into slabs of whole 16-user tiles that fit the workspace and hands each slab over as a call of its
// own: every per-user pointer advanced to the slab's first user, so the kernels know nothing of slabs):
//   recommend_mv_wide_score_kernel  grid (16-user tile, chunk of PFO_REC_CHUNK candidates).  The opening and stage A of the
//      kernels above (rec_score_chunk: the same bits), the chunk's scores to the workspace row of every user, and y of every
//      (user, candidate) as stage B above has it (RecMvUser, rec_mv_stock, pfo_mv_value<true>), NaN where the candidate takes no
//      part.  The exclusion list is NOT applied here: another chunk's workgroup may still be writing the y it would hit.
//   recommend_mv_wide_rank_kernel   one workgroup per user, after the kernel boundary.
//      1  the exclusion list over the user's y row as NaN (rec_mv_exclude);
//      2  the admissible candidates' keys compacted into two arrays (any order): y as an order-preserving 64-bit key with
//         -0 folded onto +0 (rec_ordered64), the score as rec_ordered; n = |A(u)|;
//      3  each array sorted by an LSD radix sort, 8 bits a pass (8 + 4 passes), over ping-pong buffers of the workspace: a
//         256-bin LDS histogram, its scan, and a stable scatter 256 keys at a time - match-any by eight ballots within a
//         wavefront (as rs_scatter_kernel, csr.hip), the wavefronts' digit counts side by side in LDS;
//      4  per admissible candidate two binary searches in each sorted array: `less` = where its run of equal keys starts,
//         `equal` = the run's length - exact integers however found, so pfo_mv_avg_rank / pfo_mv_blend give the bounded
//         kernel's fused to the bit; fused replaces y in the row;
//      5  the first k of the canonical order in k rounds: the best candidate (rec_better) that comes after the previous pick.
//   Work per user: 12 passes over <= I keys, 4 log2 n search steps per candidate, k reads of the fused row.  Nothing counts pairs.
// Workspace, per user of a slab and per candidate of I rounded up to 16 (PFO_RMW_BYTES: 36): y / fused f64 (8), two y-key
// buffers u64 (8 + 8), score f32 (4), two score-key buffers u32 (4 + 4); array by array, rows of a slab side by side.
#define PFO_RMW_BYTES 36

struct RecWideWs {
  double* y;              // [users][IP]: y, then fused
  uint64_t* yk[2];        // [users][IP] each
  float* sc;              // [users][IP]
  uint32_t* sk[2];        // [users][IP] each
  int64_t IP;             // row stride: I rounded up to 16
};

// the workspace that serves `tiles` 16-user tiles in one slab
inline int64_t rec_wide_bytes(int64_t tiles, int I) { return tiles * PFO_REC_TILE * PFO_RMW_BYTES * pfo_align_up(I, 16); }

// fp64 -> unsigned with the same order (sortable_f64 of csr.hip); -0 and +0 share a key, as == has it
__device__ __forceinline__ uint64_t rec_ordered64(double y) {
  uint64_t b = (uint64_t)__double_as_longlong(y);
  if (b == 0x8000000000000000ull) b = 0ull;
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

template <int NJ>
__global__ __launch_bounds__(PFO_REC_THREADS) void recommend_mv_wide_score_kernel(const RecArgs a, const RecMvArgs m, const RecWideWs w,
                                                                                  PFO_REC_MV_TABLES) {
  const float *__restrict__ user_emb = a.user_emb, *__restrict__ item_emb = a.item_emb;
  float* __restrict__ score_out = m.score_out;
  const int I = a.I, D = a.D;
  constexpr int ICS = PFO_REC_CHUNK + 4;
  __shared__ float sc[PFO_REC_TILE * ICS];                           // 33 KB
  __shared__ int ub[PFO_REC_TILE];
  const int tid = threadIdx.x;
  const int64_t u0 = (int64_t)blockIdx.x * PFO_REC_TILE;
  const int c0 = (int)blockIdx.y * PFO_REC_CHUNK, n = min(PFO_REC_CHUNK, I - c0);   // (the grid has ceil(I / chunk) chunks: n >= 1)
  const double nan = __builtin_nan("");

  float4 uf[NJ];
  rec_user_fragments<NJ>(uf, user_emb, u0, a.U, D);
  unsigned pending = rec_block_table(ub, a, u0);
  while (pending) {
    int b;
    const unsigned members = rec_next_pass(pending, ub, b);
    __syncthreads();                                                 // the previous pass's scores have been read
    rec_score_chunk<NJ>(uf, item_emb + (int64_t)b * I * D, c0, n, I, D, sc, ICS);
    __syncthreads();
    for (int us = 0; us < PFO_REC_TILE; ++us) {
      if (!((members >> us) & 1u)) continue;                         // (the same for every thread; a row beyond U is no member)
      const int64_t u = u0 + us;
      const float* su = sc + us * ICS;
      const RecMvUser h(m, returns, day_idx, port_idx, port_len, u);
      for (int c = tid; c < n; c += PFO_REC_THREADS) {
        const int g = c0 + c;
        const float s = su[c];
        w.sc[u * w.IP + g] = s;
        if (score_out) score_out[u * I + g] = s;
        const int stock = rec_mv_stock(a, cand_stock, m.n_stocks, g, h.day_ok);
        w.y[u * w.IP + g] = stock < 0 ? nan : pfo_mv_value<true>(h.dayp, stock, m.n_stocks, m.n_ret, port_idx + u * m.port_stride, h.plen, m.gamma);
      }
    }
  }
}
// WEIGHTED (pfo_recommend_mv_topk_wide_weighted): the kernel above with pfo_mv_value_weighted over the user's row of port_w.  A
// sibling, not an instantiation of one shared body: written as a body inlined into two kernels the unweighted instantiations spill
// two more SGPRs, and they are to stay what they were.
template <int NJ>
__global__ __launch_bounds__(PFO_REC_THREADS) void recommend_mv_wide_score_weighted_kernel(const RecArgs a, const RecMvArgs m, const RecWideWs w,
                                                                                           PFO_REC_MV_TABLES, const double* __restrict__ port_w) {
  const float *__restrict__ user_emb = a.user_emb, *__restrict__ item_emb = a.item_emb;
  float* __restrict__ score_out = m.score_out;
  const int I = a.I, D = a.D;
  constexpr int ICS = PFO_REC_CHUNK + 4;
  __shared__ float sc[PFO_REC_TILE * ICS];                           // 33 KB
  __shared__ int ub[PFO_REC_TILE];
  const int tid = threadIdx.x;
  const int64_t u0 = (int64_t)blockIdx.x * PFO_REC_TILE;
  const int c0 = (int)blockIdx.y * PFO_REC_CHUNK, n = min(PFO_REC_CHUNK, I - c0);   // (the grid has ceil(I / chunk) chunks: n >= 1)
  const double nan = __builtin_nan("");

  float4 uf[NJ];
  rec_user_fragments<NJ>(uf, user_emb, u0, a.U, D);
  unsigned pending = rec_block_table(ub, a, u0);
  while (pending) {
    int b;
    const unsigned members = rec_next_pass(pending, ub, b);
    __syncthreads();                                                 // the previous pass's scores have been read
    rec_score_chunk<NJ>(uf, item_emb + (int64_t)b * I * D, c0, n, I, D, sc, ICS);
    __syncthreads();
    for (int us = 0; us < PFO_REC_TILE; ++us) {
      if (!((members >> us) & 1u)) continue;                         // (the same for every thread; a row beyond U is no member)
      const int64_t u = u0 + us;
      const float* su = sc + us * ICS;
      const RecMvUser h(m, returns, day_idx, port_idx, port_len, u);
      for (int c = tid; c < n; c += PFO_REC_THREADS) {
        const int g = c0 + c;
        const float s = su[c];
        w.sc[u * w.IP + g] = s;
        if (score_out) score_out[u * I + g] = s;
        const int stock = rec_mv_stock(a, cand_stock, m.n_stocks, g, h.day_ok);
        w.y[u * w.IP + g] = stock < 0 ? nan
                                      : pfo_mv_value_weighted(h.dayp, stock, m.n_stocks, m.n_ret, port_idx + u * m.port_stride,
                                                              port_w + u * m.port_stride, h.plen, m.gamma);
      }
    }
  }
}

// the first position of sorted key[0, n) that holds a key >= v (UPPER: > v)
template <bool UPPER, class K>
__device__ __forceinline__ int rec_wide_bound(const K* key, int n, K v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const K kv = key[mid];
    if (UPPER ? kv <= v : kv < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// key[0, n) of buf[0] sorted ascending in place, buf[1] the other half of the ping-pong (BYTES passes, an even number).  All
// threads of the workgroup; starts and ends on a barrier.  base[256], cnt[2][4][256]: LDS.
template <int BYTES, class K>
__device__ __forceinline__ void rec_wide_sort(K* const (&buf)[2], int n, int* base, int (*cnt)[PFO_REC_THREADS / 64][256], int* wave_tot) {
  static_assert(BYTES % 2 == 0, "the sorted keys must end in buf[0]");
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int pass = 0; pass < BYTES; ++pass) {
    const K* in = buf[pass & 1];
    K* out = buf[(pass & 1) ^ 1];
    const int shift = 8 * pass;
    // ---- histogram of the digit (a thread is a bin from here on: 256 of each)
    base[tid] = 0;
#pragma unroll
    for (int wv = 0; wv < PFO_REC_THREADS / 64; ++wv) cnt[0][wv][tid] = cnt[1][wv][tid] = 0;
    __syncthreads();                                                 // (and the previous pass's keys are all in `in`)
    for (int i = tid; i < n; i += PFO_REC_THREADS) atomicAdd(&base[(int)((in[i] >> shift) & 255)], 1);
    __syncthreads();
    // ---- exclusive scan of the 256 bins
    const int mine = base[tid];
    int incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int v = __shfl_up(incl, off, 64);
      if (lane >= off) incl += v;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int before = 0;
#pragma unroll
    for (int wv = 0; wv < PFO_REC_THREADS / 64; ++wv) before += wv < wave ? wave_tot[wv] : 0;
    base[tid] = before + incl - mine;
    __syncthreads();
    // ---- stable scatter, 256 keys at a time: a key goes to base[digit] + the earlier keys of the step with its digit
    K next = tid < n ? in[tid] : (K)0;
    for (int t0 = 0, step = 0; t0 < n; t0 += PFO_REC_THREADS, ++step) {
      const int i = t0 + tid;
      const bool live = i < n;
      const K key = next;
      if (i + PFO_REC_THREADS < n) next = in[i + PFO_REC_THREADS];  // (the next step's key is under way across the barriers)
      const int d = live ? (int)((key >> shift) & 255) : 0;
      unsigned long long same = __ballot(live);
#pragma unroll
      for (int bit = 0; bit < 8; ++bit) {
        const unsigned long long bal = __ballot(live && ((d >> bit) & 1));
        same &= ((d >> bit) & 1) ? bal : ~bal;
      }
      const int rank = __popcll(same & ((1ull << lane) - 1ull));
      int (*c)[256] = cnt[step & 1];                                 // (zero: cleared two steps ago, or above)
      if (live && rank == 0) c[wave][d] = __popcll(same);
      __syncthreads();                                               // and base has taken the previous step's counts
      if (live) {
        int off = base[d] + rank;
#pragma unroll
        for (int wv = 0; wv < PFO_REC_THREADS / 64; ++wv) off += wv < wave ? c[wv][d] : 0;
        out[off] = key;
      }
      __syncthreads();
      int total = 0;                                                 // bin tid moves on; nobody reads c again before it is written two steps on
#pragma unroll
      for (int wv = 0; wv < PFO_REC_THREADS / 64; ++wv) {
        total += c[wv][tid];
        c[wv][tid] = 0;
      }
      base[tid] += total;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(PFO_REC_THREADS) void recommend_mv_wide_rank_kernel(const RecArgs a, const RecMvArgs m, const RecWideWs w) {
  int32_t* __restrict__ top_pos = a.top_pos;
  float* __restrict__ top_score = a.top_score;
  double *__restrict__ top_fused = m.top_fused, *__restrict__ y_out = m.y_out, *__restrict__ fused_out = m.fused_out;
  const int I = a.I, k = a.k;
  const double lam = m.lam;
  __shared__ int base[256];
  __shared__ int cnt[2][PFO_REC_THREADS / 64][256];
  __shared__ int wave_tot[PFO_REC_THREADS / 64];
  __shared__ int n_adm;
  __shared__ double wave_f[2][PFO_REC_THREADS / 64];                 // the best (fused, position) of each wavefront, by round parity
  __shared__ int wave_c[2][PFO_REC_THREADS / 64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t u = blockIdx.x;                                      // (the grid is the slab's users)
  double* yv = w.y + u * w.IP;                                       // the rows are this workgroup's alone
  const float* su = w.sc + u * w.IP;
  uint64_t* const yk[2] = {w.yk[0] + u * w.IP, w.yk[1] + u * w.IP};
  uint32_t* const sk[2] = {w.sk[0] + u * w.IP, w.sk[1] + u * w.IP};
  const double nan = __builtin_nan("");

  // ---- 1: the exclusion list (every y of the row was written by the kernel before this one)
  if (tid == 0) n_adm = 0;
  rec_mv_exclude(yv, a, u);
  // ---- 2: the keys of the admissible candidates, compacted
  for (int c0 = 0; c0 < I; c0 += PFO_REC_THREADS) {
    const int c = c0 + tid;
    const double y = c < I ? yv[c] : nan;
    if (c < I && y_out) y_out[u * I + c] = y;
    const bool adm = y == y;
    const unsigned long long bal = __ballot(adm);
    int at = 0;
    if (lane == 0 && bal) at = atomicAdd(&n_adm, __popcll(bal));
    at = __shfl(at, 0, 64) + __popcll(bal & ((1ull << lane) - 1ull));
    if (adm) {
      yk[0][at] = rec_ordered64(y);
      sk[0][at] = rec_ordered(su[c]);
    }
  }
  __syncthreads();
  const int n = n_adm;
  // ---- 3: both sorted
  rec_wide_sort<8>(yk, n, base, cnt, wave_tot);
  rec_wide_sort<4>(sk, n, base, cnt, wave_tot);
  // ---- 4: ranks by position in the sorted rows, blended; fused replaces y (a thread reads and writes its own candidates)
  for (int c = tid; c < I; c += PFO_REC_THREADS) {
    const double y = yv[c];
    double f = nan;
    if (y == y) {
      const uint64_t ky = rec_ordered64(y);
      const uint32_t ks = rec_ordered(su[c]);
      const int ly = rec_wide_bound<false>(yk[0], n, ky), ey = rec_wide_bound<true>(yk[0], n, ky) - ly;
      const int ls = rec_wide_bound<false>(sk[0], n, ks), es = rec_wide_bound<true>(sk[0], n, ks) - ls;
      f = pfo_mv_blend(pfo_mv_avg_rank(ly, ey), pfo_mv_avg_rank(ls, es), lam);   // main.py:282-286
    }
    yv[c] = f;
    if (fused_out) fused_out[u * I + c] = f;
  }
  __syncthreads();
  // ---- 5: the first k of the canonical order, one a round: the best of those that come after the previous pick
  double pf = 0.0;
  int pc = -1, n_pick = 0;
  const int rounds = min(k, n);
  for (int rd = 0; rd < rounds; ++rd) {
    double bf = 0.0;
    int bc = -1;
    for (int c = tid; c < I; c += PFO_REC_THREADS) {
      const double f = yv[c];
      if (!(f == f) || (pc >= 0 && !rec_better(pf, pc, f, c))) continue;
      if (rec_better(f, c, bf, bc)) {
        bf = f;
        bc = c;
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const double of = __shfl_xor(bf, off, 64);
      const int oc = __shfl_xor(bc, off, 64);
      if (oc >= 0 && rec_better(of, oc, bf, bc)) {
        bf = of;
        bc = oc;
      }
    }
    if (lane == 0) {
      wave_f[rd & 1][wave] = bf;
      wave_c[rd & 1][wave] = bc;
    }
    __syncthreads();                                                 // (the slots of this parity are written again two rounds on)
    bf = wave_f[rd & 1][0];
    bc = wave_c[rd & 1][0];
#pragma unroll
    for (int wv = 1; wv < PFO_REC_THREADS / 64; ++wv) {
      const double of = wave_f[rd & 1][wv];
      const int oc = wave_c[rd & 1][wv];
      if (oc >= 0 && rec_better(of, oc, bf, bc)) {
        bf = of;
        bc = oc;
      }
    }
    if (bc < 0) break;                                               // nobody is left (the same for every thread)
    if (tid == 0) {
      const float sv = su[bc];
      top_pos[u * k + rd] = bc;
      top_score[u * k + rd] = sv == 0.f ? 0.f : sv;                  // a zero score is handed out as +0
      top_fused[u * k + rd] = bf;
    }
    pf = bf;
    pc = bc;
    ++n_pick;
  }
  rec_mv_empty_slots(top_pos, top_score, top_fused, a.n_valid, u, k, n_pick);
}

// ---------------------------------------------------------------------------------------------
// The list form: every user ranks a list of its own - list_pos[u, 0:list_len[u]], at most PFO_RECOMMEND_LIST_MAX_WIDTH candidate
// positions - by score or in the mean-variance order (MV), in one launch.  W D multiply-adds per user instead of I D, and I is
// bounded by nothing but the position's 31 bits: only the list is scored and ranked.
// One wavefront per user, four users per workgroup; everything a user needs lives in its wavefront's quarter of LDS (slot s of
// the list belongs to lane s & 63).  The wavefronts of a workgroup share nothing but the barriers, which stand outside every
// data-dependent branch (a wavefront beyond U walks through them with an empty list).
//   1  staging.  The row into LDS, -1 where the entry counts for nothing (beyond the length, outside [0, I), item_ok); then each
//      lane settles "first occurrence" for its at most four slots by a walk over the entries before them - a position named twice
//      counts once, for the selection and for both ranks.  MV: y of the slot in fp64 by the slot's lane (RecMvUser, rec_mv_stock,
//      pfo_mv_value<true>: the bounded kernel's calls), a NaN y leaves the list as well.
//   2  scores.  Sixteen slots a pass, four lanes per candidate row: lane (c, q) reads 16-byte pieces q, q + 4, ... of the row of
//      slot 16 t + c and holds the same pieces of the user row in registers; four fp32 partial sums per lane (fmaf), added, then
//      across the four lanes.  NOT the matrix-core order of rec_score_tile: the contract of a score here is the any-order fp32
//      dot-product bound, and both forms of this kernel run this one sequence, so they agree with each other to the bit.
//   3  plain: k rounds of a wave-wide maximum over the 64-bit keys (rec_ordered | position), as recommend_topk_kernel.
//      MV: average-tie ranks of y and of the score by counting over the list in LDS (NaN where a slot is out: every comparison
//      is false), pfo_mv_blend, and each slot's place by counting once more (rec_better); places below k write the output row.
// LDS: 2 KB per user (positions, scores), MV 4 KB more (y, fused): 8 / 24 KB a workgroup.
#define PFO_RL_USERS (PFO_REC_THREADS / 64)                  // users per workgroup
#define PFO_RL_SLOTS (PFO_RECOMMEND_LIST_MAX_WIDTH / 64)     // list slots per lane

struct RecListArgs {
  const int32_t *list_pos, *list_len;
  int list_stride;
};

template <int NJ, bool MV, bool WEIGHTED = false>
__device__ __forceinline__ void recommend_list_body(const RecArgs& a, const RecMvArgs& m, const RecListArgs& l, PFO_REC_MV_TABLES,
                                                    const double* __restrict__ port_w = nullptr) {
  static_assert(MV || !WEIGHTED, "weights weigh on y alone");
  const float *__restrict__ user_emb = a.user_emb, *__restrict__ item_emb = a.item_emb;
  const int32_t* __restrict__ list_pos = l.list_pos;
  const uint8_t* __restrict__ item_ok = a.item_ok;
  int32_t* __restrict__ top_pos = a.top_pos;
  float *__restrict__ top_score = a.top_score, *__restrict__ score_out = m.score_out;
  const int I = a.I, D = a.D, k = a.k, W = l.list_stride;
  constexpr int LW = PFO_RECOMMEND_LIST_MAX_WIDTH;
  __shared__ int lp[PFO_RL_USERS][LW];                               // the position of a slot, -1: the slot is out
  __shared__ float ls[PFO_RL_USERS][LW];                             // its score (NaN where it is out)
  __shared__ double ly[MV ? PFO_RL_USERS : 1][MV ? LW : 1];          // its y
  __shared__ double lf[MV ? PFO_RL_USERS : 1][MV ? LW : 1];          // its fused
  __shared__ int n_of[PFO_RL_USERS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t u_first = ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * PFO_RL_USERS, u = u_first + wave;
  const bool live = u < a.U;
  const int64_t ur = live ? u : a.U - 1;                             // (the row a wavefront beyond U reads; it writes nothing)
  int* const wp = lp[wave];
  float* const ws = ls[wave];
  const float nanf = __builtin_nanf("");

  // this lane's pieces of the user row: 16-byte pieces q, q + 4, ... (NJ of them cover D <= 16 NJ floats)
  const int q = lane & 3;
  float4 uf[NJ];
  {
    const float4* up = reinterpret_cast<const float4*>(user_emb + ur * D);
#pragma unroll
    for (int j = 0; j < NJ; ++j) uf[j] = 16 * j + 4 * q < D ? up[4 * j + q] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const int b = a.user_block ? min(max(a.user_block[ur], 0), a.n_t - 1) : 0;
  const float* items = item_emb + (int64_t)b * I * D;

  // ---- 1: the list
  const int n = live ? min(max(l.list_len[u], 0), W) : 0;
  int mine[PFO_RL_SLOTS];
#pragma unroll
  for (int s4 = 0; s4 < PFO_RL_SLOTS; ++s4) {
    const int s = lane + 64 * s4;
    int p = -1;
    if (s < n) {
      p = list_pos[u * W + s];
      if (p < 0 || p >= I || (item_ok && !item_ok[p])) p = -1;
    }
    mine[s4] = p;
    wp[s] = p;
  }
  __syncthreads();
  {
    unsigned dup = 0;                                                // bit s4: an earlier slot names the same position
    for (int j = 0; j < n; ++j) {
      const int pj = wp[j];
#pragma unroll
      for (int s4 = 0; s4 < PFO_RL_SLOTS; ++s4) dup |= (pj == mine[s4] && j < lane + 64 * s4 ? 1u : 0u) << s4;
    }
#pragma unroll
    for (int s4 = 0; s4 < PFO_RL_SLOTS; ++s4)
      if ((dup >> s4) & 1u) mine[s4] = -1;
  }
  double yv[PFO_RL_SLOTS];
  if constexpr (MV) {
    const RecMvUser h(m, returns, day_idx, port_idx, port_len, ur);
#pragma unroll
    for (int s4 = 0; s4 < PFO_RL_SLOTS; ++s4) {
      yv[s4] = __builtin_nan("");
      if (mine[s4] < 0) continue;
      const int stock = rec_mv_stock(a, cand_stock, m.n_stocks, mine[s4], h.day_ok);
      if constexpr (WEIGHTED) {
        if (stock >= 0)
          yv[s4] = pfo_mv_value_weighted(h.dayp, stock, m.n_stocks, m.n_ret, port_idx + ur * m.port_stride, port_w + ur * m.port_stride,
                                         h.plen, m.gamma);
      } else {
        if (stock >= 0) yv[s4] = pfo_mv_value<true>(h.dayp, stock, m.n_stocks, m.n_ret, port_idx + ur * m.port_stride, h.plen, m.gamma);
      }
      if (!(yv[s4] == yv[s4])) mine[s4] = -1;
    }
  }
  __syncthreads();                                                   // every entry of the row has been compared
#pragma unroll
  for (int s4 = 0; s4 < PFO_RL_SLOTS; ++s4) {
    const int s = lane + 64 * s4;
    wp[s] = mine[s4];
    if constexpr (MV) ly[wave][s] = yv[s4];
  }
  __syncthreads();

  // ---- 2: scores, sixteen slots a pass
  for (int s0 = 0; s0 < n; s0 += 16) {
    const int s = s0 + (lane >> 2);                                  // (s0 <= 240: inside the row)
    const int p = wp[s];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p >= 0) {
      const float4* ip = reinterpret_cast<const float4*>(items + (int64_t)p * D);
      float4 v[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) v[j] = 16 * j + 4 * q < D ? ip[4 * j + q] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        acc.x = fmaf(uf[j].x, v[j].x, acc.x);
        acc.y = fmaf(uf[j].y, v[j].y, acc.y);
        acc.z = fmaf(uf[j].z, v[j].z, acc.z);
        acc.w = fmaf(uf[j].w, v[j].w, acc.w);
      }
    }
    float sum = (acc.x + acc.y) + (acc.z + acc.w);
    sum += __shfl_xor(sum, 1, 64);
    sum += __shfl_xor(sum, 2, 64);
    if (q == 0) ws[s] = p >= 0 ? sum : nanf;
  }
  __syncthreads();

  // ---- 3
  if constexpr (!MV) {
    unsigned long long key[PFO_RL_SLOTS];
#pragma unroll
    for (int s4 = 0; s4 < PFO_RL_SLOTS; ++s4) {
      const int s = lane + 64 * s4;
      const bool in = mine[s4] >= 0;
      const float sv = in ? ws[s] : nanf;
      key[s4] = in ? ((unsigned long long)rec_ordered(sv) << 32) | (unsigned)mine[s4] : 0ull;
      if (score_out && live && s < W) score_out[u * W + s] = sv;
    }
    unsigned long long won = 0ull;                                   // lane t: rank t
    for (int t = 0; t < k; ++t) {
      unsigned long long best = key[0];
#pragma unroll
      for (int s4 = 1; s4 < PFO_RL_SLOTS; ++s4) best = rec_max(best, key[s4]);
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) best = rec_max(best, __shfl_xor(best, off, 64));
      if (best == 0ull) break;                                       // (the same for the whole wavefront; no barrier follows)
      // positions are distinct, so exactly one key of the wavefront equals the winner: its owner clears it
#pragma unroll
      for (int s4 = 0; s4 < PFO_RL_SLOTS; ++s4)
        if (key[s4] == best) key[s4] = 0ull;
      if (lane == t) won = best;
    }
    const bool got = lane < k && won != 0ull;
    const int cnt = __popcll(__ballot(got));
    if (live) {
      if (lane < k) {
        top_pos[u * k + lane] = got ? (int32_t)(uint32_t)(won & 0xffffffffull) : -1;
        top_score[u * k + lane] = got ? rec_unordered((uint32_t)(won >> 32)) : -__builtin_inff();
      }
      if (lane == 0 && a.n_valid) a.n_valid[u] = cnt;
    }
  } else {
    double *__restrict__ top_fused = m.top_fused, *__restrict__ y_out = m.y_out, *__restrict__ fused_out = m.fused_out;
    const double* wy = ly[wave];
    double* wf = lf[wave];
    double fused[PFO_RL_SLOTS];
    int cnt = 0;
#pragma unroll
    for (int s4 = 0; s4 < PFO_RL_SLOTS; ++s4) {
      const int s = lane + 64 * s4;
      const bool in = mine[s4] >= 0;
      cnt += __popcll(__ballot(in));
      fused[s4] = __builtin_nan("");
      if (in) {
        const double yi = yv[s4];
        const float si = ws[s];
        int ly_ = 0, ey = 0, ls_ = 0, es = 0;
        for (int j = 0; j < n; ++j) {                                // (a slot that is out holds NaN in both)
          const double yj = wy[j];
          const float sj = ws[j];
          ly_ += (yj < yi);
          ey += (yj == yi);
          ls_ += (sj < si);
          es += (sj == si);                                          // (-0 == +0)
        }
        fused[s4] = pfo_mv_blend(pfo_mv_avg_rank(ly_, ey), pfo_mv_avg_rank(ls_, es), m.lam);   // main.py:282-286
      }
      wf[s] = fused[s4];
      if (live && s < W) {
        if (score_out) score_out[u * W + s] = in ? ws[s] : nanf;
        if (y_out) y_out[u * W + s] = yv[s4];
        if (fused_out) fused_out[u * W + s] = fused[s4];
      }
    }
    if (lane == 0) n_of[wave] = min(k, cnt);
    __syncthreads();
#pragma unroll
    for (int s4 = 0; s4 < PFO_RL_SLOTS; ++s4) {
      const double fi = fused[s4];
      if (!(fi == fi)) continue;                                     // (out, or a NaN blend: lambda_mv is the caller's)
      const int c = mine[s4];
      int before = 0;
      for (int j = 0; j < n; ++j) {
        const double fj = wf[j];
        before += rec_better(fj, wp[j], fi, c);                       // (false for the slot itself, and for a NaN)
      }
      if (before < k) {
        const float sv = ws[lane + 64 * s4];
        top_pos[u * k + before] = c;
        top_score[u * k + before] = sv == 0.f ? 0.f : sv;            // a zero score is handed out as +0
        top_fused[u * k + before] = fi;
      }
    }
    for (int w = 0; w < PFO_RL_USERS; ++w)                           // the tail of each user's row, by the whole workgroup
      if (u_first + w < a.U) rec_mv_empty_slots(top_pos, top_score, top_fused, a.n_valid, u_first + w, k, n_of[w]);
  }
}

template <int NJ>
__global__ __launch_bounds__(PFO_REC_THREADS) void recommend_list_topk_kernel(const RecArgs a, const RecMvArgs m, const RecListArgs l,
                                                                              PFO_REC_MV_TABLES) {
  recommend_list_body<NJ, false>(a, m, l, cand_stock, returns, day_idx, port_idx, port_len);
}
template <int NJ>
__global__ __launch_bounds__(PFO_REC_THREADS) void recommend_list_mv_topk_kernel(const RecArgs a, const RecMvArgs m, const RecListArgs l,
                                                                                 PFO_REC_MV_TABLES) {
  recommend_list_body<NJ, true>(a, m, l, cand_stock, returns, day_idx, port_idx, port_len);
}
template <int NJ>
__global__ __launch_bounds__(PFO_REC_THREADS) void recommend_list_mv_topk_weighted_kernel(const RecArgs a, const RecMvArgs m, const RecListArgs l,
                                                                                          PFO_REC_MV_TABLES, const double* __restrict__ port_w) {
  recommend_list_body<NJ, true, true>(a, m, l, cand_stock, returns, day_idx, port_idx, port_len, port_w);
}

// ---------------------------------------------------------------------------------------------
// Host side.  The checks speak in the name of the entry that called them (`who`), as PFO_REQUIRE does with __func__.
#define PFO_REC_REQUIRE(cond, msg) \
  do { if (!(cond)) { pfo_set_error("%s: %s", who, msg); return PFO_ERR_INVALID; } } while (0)

// `items_msg` names the bound `max_items` on I, `stride_msg` the strides the entry has; rec_check_mv runs it first
int rec_check_common(const char* who, const RecArgs& a, int max_items, const char* items_msg, const char* stride_msg) {
  PFO_REC_REQUIRE(a.U >= 0 && a.U <= (int64_t)PFO_REC_TILE * 0x7fffffff, "U out of range");
  PFO_REC_REQUIRE(a.D > 0 && a.D % 4 == 0, "D must be a positive multiple of 4");
  PFO_REC_REQUIRE(a.D <= 256, "D must be at most 256");
  PFO_REC_REQUIRE(a.k >= 1 && a.k <= 64, "k must be in [1, 64]");
  PFO_REC_REQUIRE(a.I >= 1 && a.I <= max_items, items_msg);
  PFO_REC_REQUIRE(a.n_t >= 1 && (int64_t)a.n_t * a.I <= 0x7fffffff, "n_t must be at least 1 and n_t * I fit 31 bits");
  PFO_REC_REQUIRE(a.excl_stride >= 0, stride_msg);
  if (a.U == 0) return PFO_OK;                                       // (nothing is read or written: no pointer is looked at)
  PFO_REC_REQUIRE(a.user_emb && a.item_emb && a.top_pos && a.top_score, "null input or output");
  PFO_REC_REQUIRE(!a.excl_pos || a.excl_stride == 0 || a.excl_len, "excl_pos without excl_len");
  PFO_REC_REQUIRE((((uintptr_t)a.user_emb | (uintptr_t)a.item_emb) & 15) == 0, "user_emb and item_emb must be 16-byte aligned");
  return PFO_OK;
}

// the bounds of the mean-variance side (the list form runs them ahead of rec_check_mv too: rec_check_common ends on pointers)
#define PFO_REC_MV_STRIDE_MSG "excl_stride and port_stride must not be negative"
int rec_check_mv_bounds(const char* who, const RecMvArgs& m) {
  PFO_REC_REQUIRE(m.port_stride >= 0, PFO_REC_MV_STRIDE_MSG);
  PFO_REC_REQUIRE(m.n_ret >= 2 && m.n_ret <= 128, "n_ret must be in [2, 128]");
  PFO_REC_REQUIRE(m.n_days > 0 && m.n_stocks > 0, "n_days and n_stocks must be positive");
  return PFO_OK;
}

// (`max_items` / `items_msg`: the bounded kernels' bound unless the entry names its own)
int rec_check_mv(const char* who, const RecArgs& a, const RecMvArgs& m, PFO_REC_MV_TABLES, int max_items = PFO_RECOMMEND_MV_MAX_ITEMS,
                 const char* items_msg = "I must be in [1, PFO_RECOMMEND_MV_MAX_ITEMS]") {
  int rc = rec_check_common(who, a, max_items, items_msg, PFO_REC_MV_STRIDE_MSG);
  if (rc != PFO_OK) return rc;
  rc = rec_check_mv_bounds(who, m);
  if (rc != PFO_OK) return rc;
  if (a.U == 0) return PFO_OK;
  PFO_REC_REQUIRE(m.top_fused, "null input or output");
  PFO_REC_REQUIRE(cand_stock && returns && day_idx, "null mean-variance input");
  PFO_REC_REQUIRE(!port_idx || m.port_stride == 0 || port_len, "port_idx without port_len");
  return PFO_OK;
}

// the weighted entries' row (U > 0), behind rec_check_mv: weights weigh on holdings
int rec_check_weights(const char* who, const double* port_w, const int32_t* port_idx, int port_stride) {
  PFO_REC_REQUIRE(!port_w || port_stride == 0 || port_idx, "port_w without port_idx");
  return PFO_OK;
}

// the wide form's workspace (U > 0): at least one tile's worth, aligned for its fp64 rows
int rec_check_wide(const char* who, const RecArgs& a, const void* workspace, int64_t workspace_bytes) {
  PFO_REC_REQUIRE(workspace, "null workspace");
  PFO_REC_REQUIRE(workspace_bytes >= rec_wide_bytes(1, a.I), "workspace shorter than pfo_recommend_mv_wide_workspace_bytes(min(U, 16), I)");
  PFO_REC_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
  return PFO_OK;
}

// the list form's own bound, ahead of the common checks (which end on the pointers), and its rows (U > 0), behind them
int rec_check_list_stride(const char* who, int list_stride) {
  PFO_REC_REQUIRE(list_stride >= 1 && list_stride <= PFO_RECOMMEND_LIST_MAX_WIDTH, "list_stride must be in [1, PFO_RECOMMEND_LIST_MAX_WIDTH]");
  return PFO_OK;
}
// the capped forms' own bound, ahead of the common checks (which end on the pointers), and their group row (U > 0), behind them
int rec_check_cap(const char* who, int group_cap) {
  PFO_REC_REQUIRE(group_cap >= 1, "group_cap must be at least 1");
  return PFO_OK;
}
int rec_check_groups(const char* who, const int32_t* cand_group) {
  PFO_REC_REQUIRE(cand_group, "null cand_group");
  return PFO_OK;
}
// the _held forms' own bound, with the cap's, and their rows (U > 0), with the group row
int rec_check_held_stride(const char* who, int held_stride) {
  PFO_REC_REQUIRE(held_stride >= 0 && held_stride <= PFO_RECOMMEND_HELD_MAX_WIDTH, "held_stride must be in [0, PFO_RECOMMEND_HELD_MAX_WIDTH]");
  return PFO_OK;
}
int rec_check_held_rows(const char* who, const int32_t* held_group, const int32_t* held_len, int held_stride) {
  PFO_REC_REQUIRE(held_stride == 0 || (held_group && held_len), "null held_group or held_len");
  return PFO_OK;
}
int rec_check_list_rows(const char* who, const int32_t* list_pos, const int32_t* list_len) {
  PFO_REC_REQUIRE(list_pos && list_len, "null list_pos or list_len");
  return PFO_OK;
}
#undef PFO_REC_REQUIRE

constexpr size_t rec_score_bytes(int IC) { return (size_t)PFO_REC_TILE * (IC + 4) * sizeof(float); }   // sc[16][IC + 4]
// the mean-variance kernels hold every candidate of a block at once, and y[IC] in fp64 before the scores
inline int rec_mv_ic(int I) { return (int)pfo_align_up(I, 16); }
constexpr size_t rec_mv_bytes(int IC) { return (size_t)IC * sizeof(double) + rec_score_bytes(IC); }
constexpr size_t rec_group_bytes(int IC) { return (size_t)IC * sizeof(int32_t); }   // grp[IC] of a capped kernel, behind the rest
// the held-group rows of a _held kernel, behind grp: `rows` of them (the plain kernel holds hg and hc of its 16 users, the other
// two the row of the user being served)
constexpr size_t rec_held_bytes(int rows, int held_stride) { return (size_t)rows * held_stride * sizeof(int32_t); }

// One workgroup per 16 users of a kernel template (times `grid_y`: the wide form's candidate chunks), in the instantiation that
// covers a row of a.D floats, with `shmem` bytes of LDS.  `kernel_of` (PFO_REC_KERNEL) names the template: it maps
// std::integral_constant<int, NJ> to the instantiation.
#define PFO_REC_KERNEL(name) [](auto nj) { return &name<decltype(nj)::value>; }
#define PFO_REC_KERNEL_CAPPED(name) [](auto nj) { return &name<decltype(nj)::value, true>; }
#define PFO_REC_KERNEL_HELD(name) [](auto nj) { return &name<decltype(nj)::value, true, true>; }
template <class KernelOf, class... Args>
int rec_launch_grid(const char* who, KernelOf kernel_of, size_t shmem, unsigned grid_y, void* stream, const RecArgs& a, const Args&... more) {
  auto launch = [&](auto nj) -> int {
    const auto kernel = kernel_of(nj);
    if (shmem > 65536) {                                             // (more than 64 KB of dynamic LDS has to be asked for, per kernel)
      const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
      if (ea != hipSuccess) {
        pfo_set_error("%s: %zu bytes of LDS refused: %s", who, shmem, hipGetErrorString(ea));
        return PFO_ERR_HIP;
      }
    }
    const dim3 grid((unsigned)pfo_ceil_div(a.U, PFO_REC_TILE), grid_y), block(PFO_REC_THREADS);
    PFO_KLAUNCH(kernel, grid, block, shmem, (hipStream_t)stream, a, more...);
    const hipError_t e = hipGetLastError();                          // (PFO_LAUNCH_CHECK, in the entry's name)
    if (e != hipSuccess) {
      pfo_set_error("%s: launch failed: %s", who, hipGetErrorString(e));
      return PFO_ERR_HIP;
    }
    return PFO_OK;
  };
  const int nj = (a.D + 15) / 16;
  if (nj <= 2) return launch(std::integral_constant<int, 2>());
  else if (nj <= 4) return launch(std::integral_constant<int, 4>());
  else if (nj <= 8) return launch(std::integral_constant<int, 8>());
  else if (nj <= 11) return launch(std::integral_constant<int, 11>());
  else return launch(std::integral_constant<int, 16>());
}
template <class KernelOf, class... Args>
int rec_launch(const char* who, KernelOf kernel_of, size_t shmem, void* stream, const RecArgs& a, const Args&... more) {
  return rec_launch_grid(who, kernel_of, shmem, 1u, stream, a, more...);
}

}  // namespace

// The argument blocks of an entry, field by name from its parameters (every entry spells them as include/pfotgn.h does).
#define PFO_REC_ARGS(ic)                                                                                                  \
  {.user_emb = user_emb, .item_emb = item_emb, .user_block = user_block, .excl_pos = excl_pos, .excl_len = excl_len,      \
   .item_ok = item_ok, .U = U, .I = I, .n_t = n_t, .D = D, .excl_stride = excl_stride, .k = k, .IC = (ic), .top_pos = top_pos, \
   .n_valid = n_valid, .top_score = top_score}
#define PFO_REC_MV_ARGS(score, y, fused)                                                                                  \
  {.n_days = n_days, .n_stocks = n_stocks, .n_ret = n_ret, .port_stride = port_stride, .gamma = gamma, .lam = lambda_mv,  \
   .top_fused = top_fused, .y_out = (y), .fused_out = (fused), .score_out = (score)}

extern "C" int pfo_recommend_topk(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U, int32_t I,
                                  int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len, int32_t excl_stride,
                                  const uint8_t* item_ok, int32_t k, int32_t* top_pos, float* top_score, int32_t* n_valid,
                                  void* stream) {
  const RecArgs a = PFO_REC_ARGS((int)pfo_align_up(I < PFO_REC_CHUNK ? I : PFO_REC_CHUNK, 16));
  const int rc = rec_check_common(__func__, a, PFO_RECOMMEND_MAX_ITEMS, "I must be in [1, PFO_RECOMMEND_MAX_ITEMS]",
                                  "excl_stride must not be negative");
  if (rc != PFO_OK || U == 0) return rc;
  return rec_launch(__func__, PFO_REC_KERNEL(recommend_topk_kernel), rec_score_bytes(a.IC) + (size_t)a.IC, stream, a);   // (+ ok[IC])
}

extern "C" int pfo_recommend_mv_topk(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U, int32_t I,
                                     int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len, int32_t excl_stride,
                                     const uint8_t* item_ok, const int32_t* cand_stock, const double* returns, int32_t n_days,
                                     int32_t n_stocks, int32_t n_ret, const int32_t* day_idx, const int32_t* port_idx,
                                     const int32_t* port_len, int32_t port_stride, double gamma, double lambda_mv, int32_t k,
                                     int32_t* top_pos, float* top_score, double* top_fused, int32_t* n_valid, float* score_out,
                                     double* y_out, double* fused_out, void* stream) {
  const RecArgs a = PFO_REC_ARGS(rec_mv_ic(I));
  const RecMvArgs m = PFO_REC_MV_ARGS(score_out, y_out, fused_out);
  const int rc = rec_check_mv(__func__, a, m, cand_stock, returns, day_idx, port_idx, port_len);
  if (rc != PFO_OK || U == 0) return rc;
  return rec_launch(__func__, PFO_REC_KERNEL(recommend_mv_topk_kernel), rec_mv_bytes(a.IC), stream, a, m, cand_stock, returns, day_idx, port_idx,
                    port_len);
}

extern "C" int pfo_recommend_basket_topk(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U,
                                         int32_t I, int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len,
                                         int32_t excl_stride, const uint8_t* item_ok, const int32_t* cand_stock,
                                         const double* returns, int32_t n_days, int32_t n_stocks, int32_t n_ret,
                                         const int32_t* day_idx, const int32_t* port_idx, const int32_t* port_len,
                                         int32_t port_stride, double gamma, double lambda_mv, int32_t k, int32_t* top_pos,
                                         float* top_score, double* top_fused, int32_t* n_valid, void* stream) {
  const RecArgs a = PFO_REC_ARGS(rec_mv_ic(I));
  const RecMvArgs m = PFO_REC_MV_ARGS(nullptr, nullptr, nullptr);
  const int rc = rec_check_mv(__func__, a, m, cand_stock, returns, day_idx, port_idx, port_len);
  if (rc != PFO_OK || U == 0) return rc;
  return rec_launch(__func__, PFO_REC_KERNEL(recommend_basket_topk_kernel), rec_mv_bytes(a.IC), stream, a, m, cand_stock, returns, day_idx,
                    port_idx, port_len);
}

// The capped forms: the sibling's argument blocks and checks, the two cap arguments on top, the CAPPED instantiation.
#define PFO_REC_CAPPED_ARGS(ic)    \
  RecArgs a = PFO_REC_ARGS(ic);    \
  a.cand_group = cand_group;       \
  a.group_cap = group_cap

extern "C" int pfo_recommend_topk_capped(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U, int32_t I,
                                         int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len, int32_t excl_stride,
                                         const uint8_t* item_ok, const int32_t* cand_group, int32_t group_cap, int32_t k,
                                         int32_t* top_pos, float* top_score, int32_t* n_valid, void* stream) {
  PFO_REC_CAPPED_ARGS((int)pfo_align_up(I < PFO_REC_CHUNK ? I : PFO_REC_CHUNK, 16));
  int rc = rec_check_cap(__func__, group_cap);
  if (rc == PFO_OK)
    rc = rec_check_common(__func__, a, PFO_RECOMMEND_MAX_ITEMS, "I must be in [1, PFO_RECOMMEND_MAX_ITEMS]", "excl_stride must not be negative");
  if (rc != PFO_OK || U == 0) return rc;
  rc = rec_check_groups(__func__, cand_group);
  if (rc != PFO_OK) return rc;
  return rec_launch(__func__, PFO_REC_KERNEL_CAPPED(recommend_topk_kernel), rec_score_bytes(a.IC) + (size_t)a.IC + rec_group_bytes(a.IC), stream,
                    a);                                              // (+ ok[IC] + grp[IC])
}

extern "C" int pfo_recommend_mv_topk_capped(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U, int32_t I,
                                            int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len, int32_t excl_stride,
                                            const uint8_t* item_ok, const int32_t* cand_group, int32_t group_cap,
                                            const int32_t* cand_stock, const double* returns, int32_t n_days, int32_t n_stocks,
                                            int32_t n_ret, const int32_t* day_idx, const int32_t* port_idx, const int32_t* port_len,
                                            int32_t port_stride, double gamma, double lambda_mv, int32_t k, int32_t* top_pos,
                                            float* top_score, double* top_fused, int32_t* n_valid, float* score_out, double* y_out,
                                            double* fused_out, void* stream) {
  PFO_REC_CAPPED_ARGS(rec_mv_ic(I));
  const RecMvArgs m = PFO_REC_MV_ARGS(score_out, y_out, fused_out);
  int rc = rec_check_cap(__func__, group_cap);
  if (rc == PFO_OK) rc = rec_check_mv_bounds(__func__, m);         // (ahead of rec_check_mv, which ends on the pointers)
  if (rc == PFO_OK) rc = rec_check_mv(__func__, a, m, cand_stock, returns, day_idx, port_idx, port_len);
  if (rc != PFO_OK || U == 0) return rc;
  rc = rec_check_groups(__func__, cand_group);
  if (rc != PFO_OK) return rc;
  return rec_launch(__func__, PFO_REC_KERNEL_CAPPED(recommend_mv_topk_kernel), rec_mv_bytes(a.IC) + rec_group_bytes(a.IC), stream, a, m, cand_stock,
                    returns, day_idx, port_idx, port_len);
}

extern "C" int pfo_recommend_basket_topk_capped(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U,
                                                int32_t I, int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len,
                                                int32_t excl_stride, const uint8_t* item_ok, const int32_t* cand_group,
                                                int32_t group_cap, const int32_t* cand_stock, const double* returns, int32_t n_days,
                                                int32_t n_stocks, int32_t n_ret, const int32_t* day_idx, const int32_t* port_idx,
                                                const int32_t* port_len, int32_t port_stride, double gamma, double lambda_mv,
                                                int32_t k, int32_t* top_pos, float* top_score, double* top_fused, int32_t* n_valid,
                                                void* stream) {
  PFO_REC_CAPPED_ARGS(rec_mv_ic(I));
  const RecMvArgs m = PFO_REC_MV_ARGS(nullptr, nullptr, nullptr);
  int rc = rec_check_cap(__func__, group_cap);
  if (rc == PFO_OK) rc = rec_check_mv_bounds(__func__, m);         // (ahead of rec_check_mv, which ends on the pointers)
  if (rc == PFO_OK) rc = rec_check_mv(__func__, a, m, cand_stock, returns, day_idx, port_idx, port_len);
  if (rc != PFO_OK || U == 0) return rc;
  rc = rec_check_groups(__func__, cand_group);
  if (rc != PFO_OK) return rc;
  return rec_launch(__func__, PFO_REC_KERNEL_CAPPED(recommend_basket_topk_kernel), rec_mv_bytes(a.IC) + rec_group_bytes(a.IC), stream, a, m,
                    cand_stock, returns, day_idx, port_idx, port_len);
}

// The _held forms: the capped sibling's argument blocks and checks, the three held arguments on top, the HELD instantiation.
#define PFO_REC_HELD_ARGS(ic)      \
  PFO_REC_CAPPED_ARGS(ic);         \
  a.held_stride = held_stride;     \
  a.held_group = held_group;       \
  a.held_len = held_len

extern "C" int pfo_recommend_topk_capped_held(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U,
                                              int32_t I, int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len,
                                              int32_t excl_stride, const uint8_t* item_ok, const int32_t* cand_group, int32_t group_cap,
                                              const int32_t* held_group, const int32_t* held_len, int32_t held_stride, int32_t k,
                                              int32_t* top_pos, float* top_score, int32_t* n_valid, void* stream) {
  PFO_REC_HELD_ARGS((int)pfo_align_up(I < PFO_REC_CHUNK ? I : PFO_REC_CHUNK, 16));
  int rc = rec_check_cap(__func__, group_cap);
  if (rc == PFO_OK) rc = rec_check_held_stride(__func__, held_stride);
  if (rc == PFO_OK)
    rc = rec_check_common(__func__, a, PFO_RECOMMEND_MAX_ITEMS, "I must be in [1, PFO_RECOMMEND_MAX_ITEMS]", "excl_stride must not be negative");
  if (rc != PFO_OK || U == 0) return rc;
  rc = rec_check_groups(__func__, cand_group);
  if (rc == PFO_OK) rc = rec_check_held_rows(__func__, held_group, held_len, held_stride);
  if (rc != PFO_OK) return rc;
  return rec_launch(__func__, PFO_REC_KERNEL_HELD(recommend_topk_kernel),
                    rec_score_bytes(a.IC) + (size_t)a.IC + rec_group_bytes(a.IC) + rec_held_bytes(2 * PFO_REC_TILE, held_stride) +
                        2 * PFO_REC_TILE * sizeof(int32_t),
                    stream, a);                                      // (+ ok[IC] + grp[IC] + hg, hc[16][held_stride] + hn[32])
}

extern "C" int pfo_recommend_mv_topk_capped_held(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U,
                                                 int32_t I, int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len,
                                                 int32_t excl_stride, const uint8_t* item_ok, const int32_t* cand_group,
                                                 int32_t group_cap, const int32_t* held_group, const int32_t* held_len,
                                                 int32_t held_stride, const int32_t* cand_stock, const double* returns, int32_t n_days,
                                                 int32_t n_stocks, int32_t n_ret, const int32_t* day_idx, const int32_t* port_idx,
                                                 const int32_t* port_len, int32_t port_stride, double gamma, double lambda_mv, int32_t k,
                                                 int32_t* top_pos, float* top_score, double* top_fused, int32_t* n_valid,
                                                 float* score_out, double* y_out, double* fused_out, void* stream) {
  PFO_REC_HELD_ARGS(rec_mv_ic(I));
  const RecMvArgs m = PFO_REC_MV_ARGS(score_out, y_out, fused_out);
  int rc = rec_check_cap(__func__, group_cap);
  if (rc == PFO_OK) rc = rec_check_held_stride(__func__, held_stride);
  if (rc == PFO_OK) rc = rec_check_mv_bounds(__func__, m);         // (ahead of rec_check_mv, which ends on the pointers)
  if (rc == PFO_OK) rc = rec_check_mv(__func__, a, m, cand_stock, returns, day_idx, port_idx, port_len);
  if (rc != PFO_OK || U == 0) return rc;
  rc = rec_check_groups(__func__, cand_group);
  if (rc == PFO_OK) rc = rec_check_held_rows(__func__, held_group, held_len, held_stride);
  if (rc != PFO_OK) return rc;
  return rec_launch(__func__, PFO_REC_KERNEL_HELD(recommend_mv_topk_kernel),
                    rec_mv_bytes(a.IC) + rec_group_bytes(a.IC) + rec_held_bytes(1, held_stride), stream, a, m, cand_stock, returns, day_idx,
                    port_idx, port_len);
}

extern "C" int pfo_recommend_basket_topk_capped_held(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U,
                                                     int32_t I, int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len,
                                                     int32_t excl_stride, const uint8_t* item_ok, const int32_t* cand_group,
                                                     int32_t group_cap, const int32_t* held_group, const int32_t* held_len,
                                                     int32_t held_stride, const int32_t* cand_stock, const double* returns,
                                                     int32_t n_days, int32_t n_stocks, int32_t n_ret, const int32_t* day_idx,
                                                     const int32_t* port_idx, const int32_t* port_len, int32_t port_stride, double gamma,
                                                     double lambda_mv, int32_t k, int32_t* top_pos, float* top_score, double* top_fused,
                                                     int32_t* n_valid, void* stream) {
  PFO_REC_HELD_ARGS(rec_mv_ic(I));
  const RecMvArgs m = PFO_REC_MV_ARGS(nullptr, nullptr, nullptr);
  int rc = rec_check_cap(__func__, group_cap);
  if (rc == PFO_OK) rc = rec_check_held_stride(__func__, held_stride);
  if (rc == PFO_OK) rc = rec_check_mv_bounds(__func__, m);         // (ahead of rec_check_mv, which ends on the pointers)
  if (rc == PFO_OK) rc = rec_check_mv(__func__, a, m, cand_stock, returns, day_idx, port_idx, port_len);
  if (rc != PFO_OK || U == 0) return rc;
  rc = rec_check_groups(__func__, cand_group);
  if (rc == PFO_OK) rc = rec_check_held_rows(__func__, held_group, held_len, held_stride);
  if (rc != PFO_OK) return rc;
  return rec_launch(__func__, PFO_REC_KERNEL_HELD(recommend_basket_topk_kernel),
                    rec_mv_bytes(a.IC) + rec_group_bytes(a.IC) + rec_held_bytes(1, held_stride), stream, a, m, cand_stock, returns, day_idx,
                    port_idx, port_len);
}

extern "C" int64_t pfo_recommend_mv_wide_workspace_bytes(int64_t U, int32_t I) {
  return rec_wide_bytes(U > 0 ? pfo_ceil_div(U, PFO_REC_TILE) : 1, I > 0 ? I : 1);
}

// The wide form behind both of its entries (`who`): port_w NULL is the unweighted score kernel, else the weighted one; the rank
// kernel never sees the portfolio.
static int rec_mv_topk_wide(const char* who, const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U, int32_t I,
                            int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len, int32_t excl_stride,
                            const uint8_t* item_ok, const int32_t* cand_stock, const double* returns, int32_t n_days, int32_t n_stocks,
                            int32_t n_ret, const int32_t* day_idx, const int32_t* port_idx, const int32_t* port_len, const double* port_w,
                            int32_t port_stride, double gamma, double lambda_mv, int32_t k, int32_t* top_pos, float* top_score,
                            double* top_fused, int32_t* n_valid, float* score_out, double* y_out, double* fused_out, void* workspace,
                            int64_t workspace_bytes, void* stream) {
  const RecArgs a = PFO_REC_ARGS(PFO_REC_CHUNK);
  const RecMvArgs m = PFO_REC_MV_ARGS(score_out, y_out, fused_out);
  int rc = rec_check_mv(who, a, m, cand_stock, returns, day_idx, port_idx, port_len, PFO_RECOMMEND_MV_WIDE_MAX_ITEMS,
                        "I must be in [1, PFO_RECOMMEND_MV_WIDE_MAX_ITEMS]");
  if (rc != PFO_OK || U == 0) return rc;
  rc = rec_check_weights(who, port_w, port_idx, port_stride);
  if (rc != PFO_OK) return rc;
  if (!port_idx || port_stride == 0) port_w = nullptr;                 // (no holding is read: the unweighted kernel serves)
  rc = rec_check_wide(who, a, workspace, workspace_bytes);
  if (rc != PFO_OK) return rc;
  // slabs of as many whole tiles as the workspace holds, in stream order (which is what makes its reuse safe)
  const int64_t tiles = pfo_ceil_div(U, PFO_REC_TILE), slab_tiles = std::min(workspace_bytes / rec_wide_bytes(1, I), tiles);
  const int64_t IP = pfo_align_up(I, 16), rows = slab_tiles * PFO_REC_TILE * IP;
  RecWideWs w;
  w.IP = IP;
  w.y = static_cast<double*>(workspace);
  w.yk[0] = reinterpret_cast<uint64_t*>(w.y + rows);
  w.yk[1] = w.yk[0] + rows;
  w.sc = reinterpret_cast<float*>(w.yk[1] + rows);
  w.sk[0] = reinterpret_cast<uint32_t*>(w.sc + rows);
  w.sk[1] = w.sk[0] + rows;
  for (int64_t t0 = 0; t0 < tiles; t0 += slab_tiles) {
    const int64_t s = t0 * PFO_REC_TILE, Us = std::min(slab_tiles * PFO_REC_TILE, U - s);   // the slab: users [s, s + Us)
    RecArgs as = a;
    RecMvArgs ms = m;
    as.U = Us;
    as.user_emb += s * D;
    if (as.user_block) as.user_block += s;
    if (as.excl_pos) as.excl_pos += s * excl_stride;
    if (as.excl_len) as.excl_len += s;
    as.top_pos += s * k;
    as.top_score += s * k;
    if (as.n_valid) as.n_valid += s;
    ms.top_fused += s * k;
    if (ms.score_out) ms.score_out += s * I;
    if (ms.y_out) ms.y_out += s * I;
    if (ms.fused_out) ms.fused_out += s * I;
    const int32_t* port_s = port_idx ? port_idx + s * port_stride : nullptr;
    const int32_t* plen_s = port_len ? port_len + s : nullptr;
    if (port_w) {
      const double* pw_s = port_w + s * port_stride;
      rc = rec_launch_grid(who, PFO_REC_KERNEL(recommend_mv_wide_score_weighted_kernel), 0, (unsigned)pfo_ceil_div(I, PFO_REC_CHUNK), stream,
                           as, ms, w, cand_stock, returns, day_idx + s, port_s, plen_s, pw_s);
    } else {
      rc = rec_launch_grid(who, PFO_REC_KERNEL(recommend_mv_wide_score_kernel), 0, (unsigned)pfo_ceil_div(I, PFO_REC_CHUNK), stream, as, ms,
                           w, cand_stock, returns, day_idx + s, port_s, plen_s);
    }
    if (rc != PFO_OK) return rc;
    PFO_KLAUNCH(recommend_mv_wide_rank_kernel, dim3((unsigned)Us), dim3(PFO_REC_THREADS), 0, (hipStream_t)stream, as, ms, w);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
      pfo_set_error("%s: launch failed: %s", who, hipGetErrorString(e));
      return PFO_ERR_HIP;
    }
  }
  return PFO_OK;
}

extern "C" int pfo_recommend_mv_topk_wide(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U, int32_t I,
                                          int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len, int32_t excl_stride,
                                          const uint8_t* item_ok, const int32_t* cand_stock, const double* returns, int32_t n_days,
                                          int32_t n_stocks, int32_t n_ret, const int32_t* day_idx, const int32_t* port_idx,
                                          const int32_t* port_len, int32_t port_stride, double gamma, double lambda_mv, int32_t k,
                                          int32_t* top_pos, float* top_score, double* top_fused, int32_t* n_valid, float* score_out,
                                          double* y_out, double* fused_out, void* workspace, int64_t workspace_bytes, void* stream) {
  return rec_mv_topk_wide(__func__, user_emb, item_emb, user_block, U, I, n_t, D, excl_pos, excl_len, excl_stride, item_ok, cand_stock, returns,
                          n_days, n_stocks, n_ret, day_idx, port_idx, port_len, nullptr, port_stride, gamma, lambda_mv, k, top_pos, top_score,
                          top_fused, n_valid, score_out, y_out, fused_out, workspace, workspace_bytes, stream);
}

// The weighted entries: the sibling's argument blocks and checks, port_w behind port_len, the WEIGHTED kernel.  A null
// port_w is the sibling itself.
extern "C" int pfo_recommend_mv_topk_wide_weighted(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U,
                                                   int32_t I, int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len,
                                                   int32_t excl_stride, const uint8_t* item_ok, const int32_t* cand_stock,
                                                   const double* returns, int32_t n_days, int32_t n_stocks, int32_t n_ret,
                                                   const int32_t* day_idx, const int32_t* port_idx, const int32_t* port_len,
                                                   const double* port_w, int32_t port_stride, double gamma, double lambda_mv, int32_t k,
                                                   int32_t* top_pos, float* top_score, double* top_fused, int32_t* n_valid, float* score_out,
                                                   double* y_out, double* fused_out, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!port_w)
    return pfo_recommend_mv_topk_wide(user_emb, item_emb, user_block, U, I, n_t, D, excl_pos, excl_len, excl_stride, item_ok, cand_stock, returns,
                                      n_days, n_stocks, n_ret, day_idx, port_idx, port_len, port_stride, gamma, lambda_mv, k, top_pos, top_score,
                                      top_fused, n_valid, score_out, y_out, fused_out, workspace, workspace_bytes, stream);
  return rec_mv_topk_wide(__func__, user_emb, item_emb, user_block, U, I, n_t, D, excl_pos, excl_len, excl_stride, item_ok, cand_stock, returns,
                          n_days, n_stocks, n_ret, day_idx, port_idx, port_len, port_w, port_stride, gamma, lambda_mv, k, top_pos, top_score,
                          top_fused, n_valid, score_out, y_out, fused_out, workspace, workspace_bytes, stream);
}

extern "C" int pfo_recommend_mv_topk_weighted(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U, int32_t I,
                                              int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len, int32_t excl_stride,
                                              const uint8_t* item_ok, const int32_t* cand_stock, const double* returns, int32_t n_days,
                                              int32_t n_stocks, int32_t n_ret, const int32_t* day_idx, const int32_t* port_idx,
                                              const int32_t* port_len, const double* port_w, int32_t port_stride, double gamma,
                                              double lambda_mv, int32_t k, int32_t* top_pos, float* top_score, double* top_fused,
                                              int32_t* n_valid, float* score_out, double* y_out, double* fused_out, void* stream) {
  if (!port_w)
    return pfo_recommend_mv_topk(user_emb, item_emb, user_block, U, I, n_t, D, excl_pos, excl_len, excl_stride, item_ok, cand_stock, returns, n_days,
                                 n_stocks, n_ret, day_idx, port_idx, port_len, port_stride, gamma, lambda_mv, k, top_pos, top_score, top_fused,
                                 n_valid, score_out, y_out, fused_out, stream);
  const RecArgs a = PFO_REC_ARGS(rec_mv_ic(I));
  const RecMvArgs m = PFO_REC_MV_ARGS(score_out, y_out, fused_out);
  int rc = rec_check_mv(__func__, a, m, cand_stock, returns, day_idx, port_idx, port_len);
  if (rc != PFO_OK || U == 0) return rc;
  rc = rec_check_weights(__func__, port_w, port_idx, port_stride);
  if (rc != PFO_OK) return rc;
  if (!port_idx || port_stride == 0)                                   // (no holding is read: the unweighted kernel serves)
    return rec_launch(__func__, PFO_REC_KERNEL(recommend_mv_topk_kernel), rec_mv_bytes(a.IC), stream, a, m, cand_stock, returns, day_idx,
                      port_idx, port_len);
  return rec_launch(__func__, PFO_REC_KERNEL(recommend_mv_topk_weighted_kernel), rec_mv_bytes(a.IC), stream, a, m, cand_stock, returns, day_idx,
                    port_idx, port_len, port_w);
}

// The list form has no exclusion side: its RecArgs carry none.  Four users a workgroup, so four workgroups (grid y) to the
// launcher's 16-user column.
#define PFO_REC_LIST_ARGS()                                               \
  const int32_t *excl_pos = nullptr, *excl_len = nullptr;                 \
  const int32_t excl_stride = 0;                                          \
  const RecArgs a = PFO_REC_ARGS(0);                                      \
  const RecListArgs l = {list_pos, list_len, list_stride}

extern "C" int pfo_recommend_list_topk(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U, int32_t I,
                                       int32_t n_t, int32_t D, const int32_t* list_pos, const int32_t* list_len, int32_t list_stride,
                                       const uint8_t* item_ok, int32_t k, int32_t* top_pos, float* top_score, int32_t* n_valid,
                                       float* score_out, void* stream) {
  PFO_REC_LIST_ARGS();
  RecMvArgs m = {};
  m.score_out = score_out;
  int rc = rec_check_list_stride(__func__, list_stride);
  if (rc == PFO_OK)
    rc = rec_check_common(__func__, a, PFO_RECOMMEND_MAX_ITEMS, "I must be in [1, PFO_RECOMMEND_MAX_ITEMS]", "excl_stride must not be negative");
  if (rc != PFO_OK || U == 0) return rc;
  rc = rec_check_list_rows(__func__, list_pos, list_len);
  if (rc != PFO_OK) return rc;
  const int32_t* none = nullptr;
  const double* no_returns = nullptr;
  return rec_launch_grid(__func__, PFO_REC_KERNEL(recommend_list_topk_kernel), 0, PFO_REC_TILE / PFO_RL_USERS, stream, a, m, l, none,
                         no_returns, none, none, none);
}

extern "C" int pfo_recommend_list_mv_topk(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U, int32_t I,
                                          int32_t n_t, int32_t D, const int32_t* list_pos, const int32_t* list_len, int32_t list_stride,
                                          const uint8_t* item_ok, const int32_t* cand_stock, const double* returns, int32_t n_days,
                                          int32_t n_stocks, int32_t n_ret, const int32_t* day_idx, const int32_t* port_idx,
                                          const int32_t* port_len, int32_t port_stride, double gamma, double lambda_mv, int32_t k,
                                          int32_t* top_pos, float* top_score, double* top_fused, int32_t* n_valid, float* score_out,
                                          double* y_out, double* fused_out, void* stream) {
  PFO_REC_LIST_ARGS();
  const RecMvArgs m = PFO_REC_MV_ARGS(score_out, y_out, fused_out);
  int rc = rec_check_list_stride(__func__, list_stride);
  if (rc == PFO_OK) rc = rec_check_mv_bounds(__func__, m);
  if (rc == PFO_OK)
    rc = rec_check_mv(__func__, a, m, cand_stock, returns, day_idx, port_idx, port_len, PFO_RECOMMEND_MAX_ITEMS,
                      "I must be in [1, PFO_RECOMMEND_MAX_ITEMS]");
  if (rc != PFO_OK || U == 0) return rc;
  rc = rec_check_list_rows(__func__, list_pos, list_len);
  if (rc != PFO_OK) return rc;
  return rec_launch_grid(__func__, PFO_REC_KERNEL(recommend_list_mv_topk_kernel), 0, PFO_REC_TILE / PFO_RL_USERS, stream, a, m, l, cand_stock,
                         returns, day_idx, port_idx, port_len);
}

extern "C" int pfo_recommend_list_mv_topk_weighted(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U,
                                                   int32_t I, int32_t n_t, int32_t D, const int32_t* list_pos, const int32_t* list_len,
                                                   int32_t list_stride, const uint8_t* item_ok, const int32_t* cand_stock,
                                                   const double* returns, int32_t n_days, int32_t n_stocks, int32_t n_ret,
                                                   const int32_t* day_idx, const int32_t* port_idx, const int32_t* port_len,
                                                   const double* port_w, int32_t port_stride, double gamma, double lambda_mv, int32_t k,
                                                   int32_t* top_pos, float* top_score, double* top_fused, int32_t* n_valid, float* score_out,
                                                   double* y_out, double* fused_out, void* stream) {
  if (!port_w)
    return pfo_recommend_list_mv_topk(user_emb, item_emb, user_block, U, I, n_t, D, list_pos, list_len, list_stride, item_ok, cand_stock, returns,
                                      n_days, n_stocks, n_ret, day_idx, port_idx, port_len, port_stride, gamma, lambda_mv, k, top_pos, top_score,
                                      top_fused, n_valid, score_out, y_out, fused_out, stream);
  PFO_REC_LIST_ARGS();
  const RecMvArgs m = PFO_REC_MV_ARGS(score_out, y_out, fused_out);
  int rc = rec_check_list_stride(__func__, list_stride);
  if (rc == PFO_OK) rc = rec_check_mv_bounds(__func__, m);
  if (rc == PFO_OK)
    rc = rec_check_mv(__func__, a, m, cand_stock, returns, day_idx, port_idx, port_len, PFO_RECOMMEND_MAX_ITEMS,
                      "I must be in [1, PFO_RECOMMEND_MAX_ITEMS]");
  if (rc != PFO_OK || U == 0) return rc;
  rc = rec_check_weights(__func__, port_w, port_idx, port_stride);
  if (rc == PFO_OK) rc = rec_check_list_rows(__func__, list_pos, list_len);
  if (rc != PFO_OK) return rc;
  if (!port_idx || port_stride == 0)                                   // (no holding is read: the unweighted kernel serves)
    return rec_launch_grid(__func__, PFO_REC_KERNEL(recommend_list_mv_topk_kernel), 0, PFO_REC_TILE / PFO_RL_USERS, stream, a, m, l, cand_stock,
                           returns, day_idx, port_idx, port_len);
  return rec_launch_grid(__func__, PFO_REC_KERNEL(recommend_list_mv_topk_weighted_kernel), 0, PFO_REC_TILE / PFO_RL_USERS, stream, a, m, l,
                         cand_stock, returns, day_idx, port_idx, port_len, port_w);
}
