// The attention forward: the register kernel, the key-ring kernel with its shader-clock pair, and the dropout-mask writer
// (attn_dev.hpp has what they share with the backward files; attn.hip picks the form and brackets the launch).
#include "attn_dev.hpp"

#define FWD_WAVES(NR, H) ((NR) * (H) <= 6 ? 5 : 2)      // registers per lane the compiler may use: 96 for D <= 192 with two heads
template <int NR, int H>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(FWD_WAVES(NR, H)))) void attn_fwd_kernel(const AttnDev a) {
  // the time-encoder parameters live in LDS, not in six registers per lane: with them the kernel fits 96 registers = 5
  // wavefronts per SIMD instead of 4
  __shared__ float s_tw[NR * 64], s_tb[NR * 64];
  for (int c = threadIdx.x; c < NR * 64; c += 256) {
    s_tw[c] = c < a.D ? a.tw[c] : 0.f;
    s_tb[c] = c < a.D ? a.tb[c] : 0.f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = (int64_t)blockIdx.x * 4 + wave;     // one instance per wavefront (a grid-stride form was measured: the
  if (n >= a.N) return;                                 // loop-carried state cost 32 VGPRs = 2 waves/SIMD and 25 % of the time)
  const int D = a.D, Ef = a.Ef, K = a.K, C = 2 * D + Ef, Cp = a.Cp;   // Cp: per-head row stride (C + 2 extra columns, padded)

  float qn[H][NR], qt[H][NR], qe[H];
  const float* qk = a.QK + (a.qk_row ? (int64_t)a.qk_row[n] : n) * a.qk_ld;
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int c = lane + 64 * r;
#pragma unroll
    for (int h = 0; h < H; ++h) {
      qn[h][r] = c < D ? qk[h * Cp + c] : 0.f;
      qt[h][r] = c < D ? qk[h * Cp + D + Ef + c] : 0.f;
    }
  }
#pragma unroll
  for (int h = 0; h < H; ++h) qe[h] = lane < Ef ? qk[h * Cp + D + lane] : 0.f;

  const int64_t slot0 = n * K;
  const bool inK = lane < K;
  const int my_id = inK ? a.nbr_ids[slot0 + lane] : 0;
  const int my_row = inK ? (a.nbr_row ? a.nbr_row[slot0 + lane] : (int)(a.nbr_row_base + slot0 + lane)) : 0;
  const int my_e = inK ? a.eidx[slot0 + lane] : 0;
  const float my_dt = inK ? a.dt[slot0 + lane] : 0.f;
  const unsigned long long valid = __ballot(inK && my_id != 0);
  float* ctx = a.ctx + n * H * Cp;
  if (valid == 0ull) {
    // no valid neighbour: the reference attends to padded slot 0 and then zero-fills the attention
    // output (temporal_attention.py:60-65,84), so nothing computed here is ever observed
    if (lane == 0) a.inv[n] = 1;
    for (int c = lane; c < H * Cp; c += 64) ctx[c] = 0.f;        // includes the Σa' and valid-flag columns
    for (int c = lane; c < H * K; c += 64) a.attw[n * H * K + c] = 0.f;
    return;
  }
  if (lane == 0) a.inv[n] = 0;

  const unsigned keep = attn_keep_for(a, a.offset + (a.offset_dev ? *a.offset_dev : 0ull), n, lane);
  const float keep_scale = a.dropout_p > 0.f ? 1.f / (1.f - a.dropout_p) : 1.f;

  float m[H], l[H], ld[H], my_s[H];
  float an[H][NR], at[H][NR], ae[H];
#pragma unroll
  for (int h = 0; h < H; ++h) {
    m[h] = -INFINITY; l[h] = 0.f; ld[h] = 0.f; my_s[h] = -INFINITY; ae[h] = 0.f;
#pragma unroll
    for (int r = 0; r < NR; ++r) { an[h][r] = 0.f; at[h][r] = 0.f; }
  }

  // Software pipeline over chunks of KC_FWD keys: the rows of chunk c+1 are gathered while chunk c is scored, so a
  // wavefront pays the gather latency once per instance, not once per chunk.  Two register sets used alternately
  // (A, B): copying the prefetched set over the current one cost 38 v_mov per iteration.
  unsigned long long vm = valid;
  int jsA[KC_FWD], jsB[KC_FWD];
  float knA[KC_FWD][NR], keA[KC_FWD], knB[KC_FWD][NR], keB[KC_FWD];
  auto pick = [&](int (&jj)[KC_FWD]) {
#pragma unroll
    for (int c = 0; c < KC_FWD; ++c) {
      jj[c] = vm ? (__ffsll((long long)vm) - 1) : -1;
      vm &= vm - 1ull;
    }
  };
  auto gather = [&](const int (&jj)[KC_FWD], float (&kk)[KC_FWD][NR], float (&ee)[KC_FWD]) {
#pragma unroll
    for (int c = 0; c < KC_FWD; ++c) {
      const int j = jj[c] < 0 ? 0 : jj[c];
      const float* src = a.nbr_tab + (uint32_t)rl_i(my_row, j) * (uint32_t)a.nbr_ld;        // 32-bit element offsets (checked on the host): one scalar multiply
      const int e = rl_i(my_e, j);
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int cc = lane + 64 * r;
        kk[c][r] = (jj[c] >= 0 && (r < NR - 1 || cc < D)) ? src[cc] : 0.f;
      }
      ee[c] = (jj[c] >= 0 && lane < Ef) ? a.edge_feat[(uint32_t)e * (uint32_t)Ef + (uint32_t)lane] : 0.f;
    }
  };
  auto process = [&](const int (&js)[KC_FWD], const float (&kn)[KC_FWD][NR], const float (&ke)[KC_FWD]) {
    float kt[KC_FWD][NR], dtv[KC_FWD], arg[KC_FWD][NR];
#pragma unroll
    for (int c = 0; c < KC_FWD; ++c) dtv[c] = rl_f(my_dt, js[c] < 0 ? 0 : js[c]);
    // time encoding of the chunk: ONE out-of-range test for all its arguments (wave-wide), then the fast reduction
    bool big = false;
#pragma unroll
    for (int c = 0; c < KC_FWD; ++c)
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        arg[c][r] = pfo_time_arg(dtv[c], s_tw[lane + 64 * r], s_tb[lane + 64 * r]);
        big = big || !(fabsf(arg[c][r]) < 2.0e7f);
      }
    const bool any_big = __ballot(big) != 0ull;
    float part[KC_FWD * H];
#pragma unroll
    for (int c = 0; c < KC_FWD; ++c) {
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int cc = lane + 64 * r;
        // lanes beyond D (last r only) evaluate a harmless cosine and are masked by a select, not a branch
        const float cv = __builtin_expect(any_big, 0) ? pfo_cosf(arg[c][r]) : __builtin_amdgcn_cosf(pfo_revolutions_fast(arg[c][r]));
        kt[c][r] = (js[c] >= 0 && (r < NR - 1 || cc < D)) ? cv : 0.f;
      }
#pragma unroll
      for (int h = 0; h < H; ++h) {
        float pp = ke[c] * qe[h];
#pragma unroll
        for (int r = 0; r < NR; ++r) pp = fmaf(kn[c][r], qn[h][r], fmaf(kt[c][r], qt[h][r], pp));
        part[c * H + h] = pp;
      }
    }
    pfo_wave_sum_scalar_n<KC_FWD * H>(part);
#pragma unroll
    for (int c = 0; c < KC_FWD; ++c) {
      if (js[c] < 0) continue;
      const unsigned kb = (unsigned)rl_i((int)keep, js[c]);
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const float sc = part[c * H + h] * a.scale;
        if (lane == js[c]) my_s[h] = sc;
        // the score is wave-uniform: the running sums are rescaled only when the maximum actually moves (a scalar
        // branch, taken for the first few keys of a row), otherwise a key costs one FMA per accumulator
        if (sc > m[h]) {
          const float corr = pfo_exp_neg(m[h] - sc);
          l[h] *= corr; ld[h] *= corr; ae[h] *= corr;
#pragma unroll
          for (int r = 0; r < NR; ++r) { an[h][r] *= corr; at[h][r] *= corr; }
          m[h] = sc;
        }
        const float pr = pfo_exp_neg(sc - m[h]);
        const float pd = ((kb >> h) & 1u) ? pr * keep_scale : 0.f;
        l[h] += pr;
        ld[h] += pd;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          an[h][r] = fmaf(pd, kn[c][r], an[h][r]);
          at[h][r] = fmaf(pd, kt[c][r], at[h][r]);
        }
        ae[h] = fmaf(pd, ke[c], ae[h]);
      }
    }
  };
  pick(jsA);
  gather(jsA, knA, keA);
  while (true) {
    pick(jsB);
    if (jsB[0] >= 0) gather(jsB, knB, keB);
    process(jsA, knA, keA);
    if (jsB[0] < 0) break;
    pick(jsA);
    if (jsA[0] >= 0) gather(jsA, knA, keA);
    process(jsB, knB, keB);
    if (jsA[0] < 0) break;
  }
#pragma unroll
  for (int h = 0; h < H; ++h) {
    const float il = 1.f / l[h];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int c = lane + 64 * r;
      if (c < D) {
        ctx[h * Cp + c] = an[h][r] * il;
        ctx[h * Cp + D + Ef + c] = at[h][r] * il;
      }
    }
    if (lane < Ef) ctx[h * Cp + D + lane] = ae[h] * il;
    if (lane < K) a.attw[(n * H + h) * K + lane] = ((valid >> lane) & 1ull) ? pfo_exp_neg(my_s[h] - m[h]) * il : 0.f;
    // extra columns consumed by the merged value/out/fc1 projection: C = Σ_j a'_jh (multiplies the folded value
    // bias), C+1 = 1 on head 0 (multiplies the folded out_proj bias; absent on rows without a valid neighbour)
    if (lane < Cp - C) ctx[h * Cp + C + lane] = lane == 0 ? ld[h] * il : ((lane == 1 && h == 0) ? 1.f : 0.f);
  }
}

// ---------------------------------------------------------------------------------------------
// KEY RING (round 6).  The kernel above keeps two register sets of KC_FWD keys: with five wavefronts per SIMD that is ten gathered
// rows in flight per SIMD, and a wavefront waits out one L2 round trip per pair of keys (ten per instance: its ~13 us life is
// mostly that).  Here the gathered rows never pass through registers: ONE global_load_lds_dwordx4 per key moves [row | edge
// feature] (lanes < D/4 read the row, the next Ef/4 lanes the edge feature - the source address of an LDS-DMA load is per lane)
// into a wavefront-private ring of FWD_RING slots in LDS, FWD_RING - 2 keys ahead of the pair being scored; the pair is read
// back with three ds_read_b32 per key.  No registers are held by data in flight, so the depth is set by LDS, not by the
// register file.  Node and edge columns are one contiguous [0, D + Ef) vector on both sides (key slot and qk' row), the time
// half is formed in registers as before.  vmcnt counts the DMAs exactly: pairs are issued two at a time (an odd tail re-reads
// its last key), so the pair at the head of the ring has landed when at most 2 (pairs issued behind it) are outstanding.
constexpr int FWD_RING = 4;     // keys per wavefront's ring (even; 8 and 6 measure the same: the depth is not what binds)
#define FWD_RING_WAVES(NR, H) ((NR) * (H) <= 6 ? 6 : ((NR) * (H) <= 8 ? 4 : ((NR) * (H) <= 12 ? 3 : 2)))   // wavefronts per SIMD the register budget is cut for
// (the qk' row is read by register-bound loads in front of the ring's DMAs: 0.168 ms per step, by LDS-DMA 0.176)
// shader-clock pair 0 of pfo_shader_clock (the ring form stamps it); the device symbol and its reader share this file
__device__ unsigned long long g_attn_fwd_clock[2];
int attn_fwd_clock_read(double* out, int reset) { return attn_clock_pair_read(HIP_SYMBOL(g_attn_fwd_clock), out, reset); }
template <int NR, int H>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(FWD_RING_WAVES(NR, H)))) void attn_fwd_ring_kernel(const AttnDev a) {
  constexpr int SLOTF = NR * 64, RP = FWD_RING / 2;      // floats per ring slot; pairs the ring holds
  static_assert(FWD_RING % 2 == 0 && FWD_RING >= 2, "ring");
  __shared__ float s_tw[NR * 64], s_tb[NR * 64];
  __shared__ __align__(16) float s_ring[4][FWD_RING][SLOTF];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int D = a.D, Ef = a.Ef, K = a.K, DE = D + Ef, C = 2 * D + Ef, Cp = a.Cp;
  const bool clk_on = blockIdx.x == 0 && threadIdx.x < 64;       // (wave-uniform)
  PfoClockStamp clk;
  if (clk_on) clk = pfo_clock_begin();
  // Every first-level load of the wavefront leaves before the barrier - the time-encoder parameters for the workgroup's LDS
  // copy, this instance's slot metadata and its query row's index (clamped instance for the wavefronts behind N): ONE round
  // trip where the barrier used to separate two.
  const int64_t n = (int64_t)blockIdx.x * 4 + wave;
  const int64_t nc = n < a.N ? n : (int64_t)a.N - 1;
  const int64_t slot0 = nc * K;
  const bool inK = lane < K;
  // (clamped addresses, not predicated loads: a predicated load is its own basic block with the wait for its result at the
  //  end - the six loads then queue as six dependent round trips; straight-line, they leave together)
  const int64_t si = slot0 + min(lane, K - 1);
  const int tcol = min((int)threadIdx.x, D - 1);
  const float twr = a.tw[tcol], tbr = a.tb[tcol];
  const int id_r = a.nbr_ids[si];
  // (an optional array is read through a pointer select - any valid address when it is absent - and its value selected away
  //  behind the loads: a load under a pointer test is a basic block of its own, too)
  const int row_l = (a.nbr_row ? a.nbr_row : a.nbr_ids)[si];
  const int e_r = a.eidx[si];
  const float dt_r = a.dt[si];
  const int qrow_l = (a.qk_row ? a.qk_row : a.nbr_ids)[nc];
  const uint32_t* const offp = a.offset_dev ? reinterpret_cast<const uint32_t*>(a.offset_dev) : reinterpret_cast<const uint32_t*>(a.tw);
  const uint32_t off_lo = offp[0], off_hi = offp[1];
  const int row_r = a.nbr_row ? row_l : (int)(a.nbr_row_base + si);
  const int qrow = a.qk_row ? qrow_l : (int)nc;
  const uint64_t rng_off = a.offset + (a.offset_dev ? (((uint64_t)off_hi << 32) | off_lo) : 0ull);
  int my_id = inK ? id_r : 0, my_row = inK ? row_r : 0, my_e = inK ? e_r : 0;
  float my_dt = inK ? dt_r : 0.f;
  if (threadIdx.x < NR * 64) { const bool on = (int)threadIdx.x < D; s_tw[threadIdx.x] = on ? twr : 0.f; s_tb[threadIdx.x] = on ? tbr : 0.f; }
  // columns [D + Ef, 64 NR) of a slot are never written by a DMA (lanes behind the row's end are off): cleared once, they
  // read as zero and the dot products need no select
  float* const ring = &s_ring[wave][0][0];
  if (lane + 64 * (NR - 1) >= DE)
#pragma unroll
    for (int s = 0; s < FWD_RING; ++s) ring[s * SLOTF + lane + 64 * (NR - 1)] = 0.f;
  __syncthreads();
  if (n >= a.N) return;
  // one range test per instance (as in the run-merged backward): |fma(dt, w, b)| <= max|dt| max|w| + max|b| < 2e7 -> the fp32
  // range reduction holds for every key of the instance
  float wmax = 0.f, bmax = 0.f;
#pragma unroll
  for (int r = 0; r < NR; ++r) { wmax = fmaxf(wmax, fabsf(s_tw[lane + 64 * r])); bmax = fmaxf(bmax, fabsf(s_tb[lane + 64 * r])); }
  wmax = pfo_wave_max(wmax); bmax = pfo_wave_max(bmax);

  const unsigned long long valid = __ballot(inK && my_id != 0);
  float* ctx = a.ctx + n * H * Cp;
  if (valid == 0ull) {
    if (lane == 0) a.inv[n] = 1;
    for (int c = lane; c < H * Cp; c += 64) ctx[c] = 0.f;
    for (int c = lane; c < H * K; c += 64) a.attw[n * H * K + c] = 0.f;
    return;
  }
  const bool fast = fmaf(pfo_wave_max(fabsf(my_dt)), wmax, bmax) < 2.0e7f;     // (every register-bound load is consumed before the first DMA)
  // ---- round trip 2, all of it LDS-DMA: the instance's qk' row (no register-bound load is in flight beside the ring: the
  // compiler waits for vmcnt(0) at the first use of such a load, i.e. for every DMA behind it) and the first pairs of keys.
  // Pair p = valid keys 2p, 2p + 1 in slot order; slots (2p) % RING, (2p + 1) % RING.
  typedef __attribute__((address_space(1))) const void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  // (every value that came from a register-bound load is pinned HERE: sunk behind the first DMA, its use would wait for vmcnt(0))
  asm volatile("" : "+v"(my_row), "+v"(my_e), "+v"(my_dt), "+v"(my_id));
  // (register-bound loads of the qk' row in front of the DMAs, clamped columns: the compiler's vmcnt(0) at their first use -
  //  the top of the walk - is the wait for the first pair anyway)
  float r1[H][NR], rt[H][NR];
  {
    const float* qk = a.QK + (int64_t)qrow * a.qk_ld;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int c1 = min(lane + 64 * r, DE - 1), ct = min(lane + 64 * r, D - 1);
#pragma unroll
      for (int h = 0; h < H; ++h) { r1[h][r] = qk[h * Cp + c1]; rt[h][r] = qk[h * Cp + DE + ct]; }
    }
  }
  const int D4 = D >> 2, DE4 = DE >> 2;
  // per lane: the table it reads (row table or edge features), its row stride in bytes and its 16-byte piece of the row; the
  // per-key address is then ONE 64-bit multiply-add (base + index * stride) on a select of two wave-uniform indices
  const bool is_node = lane < D4;
  const uint64_t base_l = (is_node ? (uint64_t)(uintptr_t)a.nbr_tab : (uint64_t)(uintptr_t)a.edge_feat) + (uint64_t)((is_node ? lane : lane - D4) * 16);
  const uint32_t mul_l = is_node ? (uint32_t)a.nbr_ld * 4u : (uint32_t)Ef * 4u;
  const uint32_t node_mask = is_node ? 0xFFFFFFFFu : 0u;        // index select without a branch: e + ((row - e) & mask)
  unsigned long long vm = valid;                               // keys not yet issued
  const int nv = __popcll(valid);
  const int n_pairs = (nv + 1) >> 1;
  int issued = 0;                                              // pairs issued
  auto issue_pair = [&]() {
    int j0 = __ffsll((long long)vm) - 1;
    vm &= vm - 1ull;
    int j1 = vm ? (__ffsll((long long)vm) - 1) : j0;           // an odd tail re-reads its last key (its weight is forced to zero)
    vm &= vm - 1ull;
    const int sl = (2 * issued) % FWD_RING;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int j = c ? j1 : j0;
      const uint32_t e_s = (uint32_t)rl_i(my_e, j);
      const uint32_t idx = e_s + (((uint32_t)rl_i(my_row, j) - e_s) & node_mask);
      const uint64_t src = base_l + (uint64_t)idx * (uint64_t)mul_l;
      if (lane < DE4) __builtin_amdgcn_global_load_lds((gptr_t)(uintptr_t)src, (lptr_t)(ring + (sl + c) * SLOTF), 16, 0, 0);
    }
    issued += 1;
  };
#pragma unroll
  for (int p = 0; p < RP; ++p)
    if (p < n_pairs) issue_pair();
  const unsigned keep = attn_keep_for(a, rng_off, n, lane);
  const float keep_scale = a.dropout_p > 0.f ? 1.f / (1.f - a.dropout_p) : 1.f;
  // the first pair has landed, and with it (older) the qk' row: [node | edge] columns as one vector, the time columns as
  // another, both pre-multiplied by scale * log2(e) - a score then leaves the reduction ready for v_exp_f32 (2^x)
  pfo_wait_pairs<RP - 1>(issued - 1);
  float q1[H][NR], qt[H][NR];
  {
    const float qs = a.scale * 1.44269504088896340736f;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int c = lane + 64 * r;
#pragma unroll
      for (int h = 0; h < H; ++h) {
        q1[h][r] = c < DE ? r1[h][r] * qs : 0.f;
        qt[h][r] = c < D ? rt[h][r] * qs : 0.f;
      }
    }
  }

  float m[H], l[H], ld[H], my_s[H];                            // m, my_s: scores in log2 units
  float a1[H][NR], at[H][NR];
#pragma unroll
  for (int h = 0; h < H; ++h) {
    m[h] = -INFINITY; l[h] = 0.f; ld[h] = 0.f; my_s[h] = -INFINITY;
#pragma unroll
    for (int r = 0; r < NR; ++r) { a1[h][r] = 0.f; at[h][r] = 0.f; }
  }
  auto walk = [&](auto fast_c) {
  constexpr bool FAST = decltype(fast_c)::value;
  unsigned long long wm = valid;                               // keys not yet scored
  for (int p = 0; p < n_pairs; ++p) {
    const int js0 = __ffsll((long long)wm) - 1;
    wm &= wm - 1ull;
    const bool has1 = wm != 0ull;
    const int js1 = has1 ? (__ffsll((long long)wm) - 1) : js0;
    wm &= wm - 1ull;
    const bool more = p + RP < n_pairs;                        // the pair RP ahead exists: RP - 1 pairs stay in flight behind this one
    if (more) pfo_wait_vm<2 * (RP - 1)>(); else pfo_wait_vm<0>();
    const float* sl = ring + ((2 * p) % FWD_RING) * SLOTF;
    float kn[2][NR], kt[2][NR], dtv[2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int r = 0; r < NR; ++r) kn[c][r] = sl[c * SLOTF + lane + 64 * r];
    dtv[0] = rl_f(my_dt, js0); dtv[1] = rl_f(my_dt, js1);
    float part[2 * H];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        // (lanes beyond D carry w = b = 0: cos(0) = 1 there, against a zero query column - no select)
        const float arg = pfo_time_arg(dtv[c], s_tw[lane + 64 * r], s_tb[lane + 64 * r]);
        kt[c][r] = __builtin_amdgcn_cosf(FAST ? pfo_revolutions_fast(arg) : pfo_revolutions(arg));
      }
#pragma unroll
      for (int h = 0; h < H; ++h) {
        float pp = 0.f;
#pragma unroll
        for (int r = 0; r < NR; ++r) pp = fmaf(kn[c][r], q1[h][r], fmaf(kt[c][r], qt[h][r], pp));
        part[c * H + h] = pp;
      }
    }
    // the slots are free again (their values sit in registers): the pair RP ahead starts its trip
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (more) issue_pair();
    pfo_wave_sum_scalar_n<2 * H>(part);
    // an absent second key (odd tail) scores -inf: weight 0 in every sum, no branch
    float sc[2][H];
#pragma unroll
    for (int h = 0; h < H; ++h) { sc[0][h] = part[h]; sc[1][h] = has1 ? part[H + h] : -INFINITY; }
    // The scores are wave-uniform: the running sums are rescaled only when a maximum actually moves - ONE scalar branch per
    // pair (taken for the first pairs of a row), all heads inside it
    bool up = false;
#pragma unroll
    for (int h = 0; h < H; ++h) up = up || sc[0][h] > m[h] || sc[1][h] > m[h];
    if (up) {
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const float mn = fmaxf(m[h], fmaxf(sc[0][h], sc[1][h]));
        const float corr = __builtin_amdgcn_exp2f(m[h] - mn);     // (first pair: 2^-inf = 0 against zero sums)
        l[h] *= corr; ld[h] *= corr;
#pragma unroll
        for (int r = 0; r < NR; ++r) { a1[h][r] *= corr; at[h][r] *= corr; }
        m[h] = mn;
      }
    }
    const unsigned kb0 = (unsigned)rl_i((int)keep, js0), kb1 = (unsigned)rl_i((int)keep, js1);
    const int js1c = has1 ? js1 : -1;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const unsigned kb = c ? kb1 : kb0;
#pragma unroll
      for (int h = 0; h < H; ++h) {
        if (lane == (c ? js1c : js0)) my_s[h] = sc[c][h];
        const float pr = __builtin_amdgcn_exp2f(sc[c][h] - m[h]);
        const float pd = ((kb >> h) & 1u) ? pr * keep_scale : 0.f;
        l[h] += pr;
        ld[h] += pd;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          a1[h][r] = fmaf(pd, kn[c][r], a1[h][r]);
          at[h][r] = fmaf(pd, kt[c][r], at[h][r]);
        }
      }
    }
  }
  };
  if (fast) walk(std::true_type{}); else walk(std::false_type{});
  if (lane == 0) a.inv[n] = 0;       // (here, not in front of the DMAs: the compiler drains a store before the first LDS-DMA load)
#pragma unroll
  for (int h = 0; h < H; ++h) {
    const float il = 1.f / l[h];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int c = lane + 64 * r;
      if (c < DE) ctx[h * Cp + c] = a1[h][r] * il;
      if (c < D) ctx[h * Cp + DE + c] = at[h][r] * il;
    }
    if (lane < K) a.attw[(n * H + h) * K + lane] = ((valid >> lane) & 1ull) ? __builtin_amdgcn_exp2f(my_s[h] - m[h]) * il : 0.f;
    if (lane < Cp - C) ctx[h * Cp + C + lane] = lane == 0 ? ld[h] * il : ((lane == 1 && h == 0) ? 1.f : 0.f);
  }
  if (clk_on && lane == 0) pfo_clock_end(clk, g_attn_fwd_clock);
}

int attn_fwd_run(int form, dim3 grid, dim3 block, const AttnDev& d, hipStream_t stream) {
  bool done;
  if (form == PFO_ATTN_FORM_FWD_RING) done = attn_for_shape<ATTN_RING_MAX_NRH>(d.D, d.H, [&](auto nr, auto h) { PFO_KLAUNCH((attn_fwd_ring_kernel<nr, h>), grid, block, 0, stream, d); });
  else done = attn_for_shape<ATTN_MAX_NRH>(d.D, d.H, [&](auto nr, auto h) { PFO_KLAUNCH((attn_fwd_kernel<nr, h>), grid, block, 0, stream, d); });
  PFO_REQUIRE(done, "unsupported (D, H) combination");
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}

// the step's dropout multipliers, written out (include/pfotgn.h pfo_attn_dropout_mask): same function, same counters
__global__ void attn_dropout_mask_kernel(uint64_t seed, uint64_t offset, int64_t N, int K, int H, float p, float* __restrict__ out) {
  const float keep_scale = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const int64_t total = N * K;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = e / K;
    const int j = (int)(e - n * K);
    const unsigned keep = attn_keep_bits(seed, offset, n, j, p);
    for (int h = 0; h < H; ++h) out[(n * H + h) * K + j] = ((keep >> h) & 1u) ? keep_scale : 0.f;
  }
}
int attn_dropout_mask_run(dim3 grid, dim3 block, uint64_t seed, uint64_t offset, int64_t N, int K, int H, float p, float* out,
                          hipStream_t stream) {
  PFO_KLAUNCH(attn_dropout_mask_kernel, grid, block, 0, stream, seed, offset, N, K, H, p, out);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}
