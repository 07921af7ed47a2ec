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
        const int item = min(c0 + 16 * t + r, I - 1);                // (a column beyond I repeats the last row; never read back)
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
