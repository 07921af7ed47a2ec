// The per-instance attention backward: the register body and its key-ring twin behind six __global__ wrappers, one per
// treatment of the neighbour-row gradients (attn_dev.hpp has what they share with the other kernel files).
#include "attn_dev.hpp"

// (DMODE 3: the deterministic form of 1 - int64 fixed-point atomics into one table, attn.hpp)
// DMODE: what happens to the neighbour-row gradients - 0 none (layer 1 without memory: level-0 rows are constants),
// 1 float atomics into the rows `nbr_row` names (layer 1 over the touched-node table), 2 plain stores (layers >= 2,
// where every (instance, slot) owns its row).  A template parameter: as a run-time test it cost three scalar branch
// sequences per key inside the inner loop.
template <int NR, int H, int DMODE>
__device__ __forceinline__ void attn_bwd_body(const AttnDev& a) {
  __shared__ double s_red[4][2][NR * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int D = a.D, Ef = a.Ef, K = a.K, C = 2 * D + Ef, Cp = a.Cp;
  constexpr bool wdirect = (DMODE == 2);                // ... and their gradients are written, not accumulated
  const bool direct = (a.nbr_row == nullptr);
  float tw[NR], tb[NR];
  double dw[NR], db[NR];     // sums of terms scaled by dt ~ 1e7 with heavy cancellation: accumulate in fp64
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int c = lane + 64 * r;
    tw[r] = c < D ? a.tw[c] : 0.f;
    tb[r] = c < D ? a.tb[c] : 0.f;
    dw[r] = 0.0; db[r] = 0.0;
  }
  const float keep_scale = a.dropout_p > 0.f ? 1.f / (1.f - a.dropout_p) : 1.f;
  // DMODE 1: every XCD adds into ITS replica of the gradient table.  The eight L2s are kept coherent by hardware, so
  // float atomics from all XCDs on one table make each cache line migrate between L2s (the 500 item rows take 77 % of
  // the adds); with one replica per XCD the atomics stay in the local L2.  The XCC id only picks the replica: a wrong
  // value would cost speed, never correctness (the atomics are device-coherent either way).
  float* const d_nbr_x = (DMODE == 1) ? a.d_nbr + (int64_t)(__builtin_amdgcn_s_getreg(6164) & (a.d_nbr_nrep - 1)) * a.d_nbr_rep : a.d_nbr;   // hwreg(HW_REG_XCC_ID, 0, 4)

  for (int64_t n = (int64_t)blockIdx.x * 4 + wave; n < a.N; n += (int64_t)gridDim.x * 4) {
    float* dqk_out = a.dQK + n * H * Cp;
    const int64_t slot0 = n * K;
    const bool inK = lane < K;
    const int my_id = inK ? a.nbr_ids[slot0 + lane] : 0;
    const int my_row = inK ? (direct ? (int)(a.nbr_row_base + slot0 + lane) : a.nbr_row[slot0 + lane]) : 0;
    const int my_e = inK ? a.eidx[slot0 + lane] : 0;
    const float my_dt = inK ? a.dt[slot0 + lane] : 0.f;
    const unsigned long long valid = __ballot(inK && my_id != 0);
    if (wdirect) {
      // padded slots own a gradient row too (the buffer is reused every step): zero it
      unsigned long long im = ~valid & (K >= 64 ? ~0ull : ((1ull << K) - 1ull));
      while (im) {
        const int j = __ffsll((long long)im) - 1;
        im &= im - 1ull;
        float* dst = a.d_nbr + (a.nbr_row_base + slot0 + j) * a.d_nbr_ld;
        for (int c = lane; c < D; c += 64) dst[c] = 0.f;
      }
    }
    if (valid == 0ull) {
      for (int c = lane; c < H * Cp; c += 64) dqk_out[c] = 0.f;
      continue;
    }
    float qn[H][NR], qt[H][NR], qe[H], gn[H][NR], gt[H][NR], ge[H], t[H], dsb[H];
    float dqn[H][NR], dqt[H][NR], dqe[H];
    const float* qk = a.QK + (a.qk_row ? (int64_t)a.qk_row[n] : n) * a.qk_ld;
    const float* dc = a.dctx + n * H * Cp;
    const float* cx = a.ctx + n * H * Cp;
#pragma unroll
    for (int h = 0; h < H; ++h) {
      float part = 0.f;
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int c = lane + 64 * r;
        const bool ok = c < D;
        qn[h][r] = ok ? qk[h * Cp + c] : 0.f;
        qt[h][r] = ok ? qk[h * Cp + D + Ef + c] : 0.f;
        gn[h][r] = ok ? dc[h * Cp + c] : 0.f;
        gt[h][r] = ok ? dc[h * Cp + D + Ef + c] : 0.f;
        if (ok) part = fmaf(gn[h][r], cx[h * Cp + c], fmaf(gt[h][r], cx[h * Cp + D + Ef + c], part));
        dqn[h][r] = 0.f; dqt[h][r] = 0.f;
      }
      qe[h] = lane < Ef ? qk[h * Cp + D + lane] : 0.f;
      ge[h] = lane < Ef ? dc[h * Cp + D + lane] : 0.f;
      if (lane < Ef) part = fmaf(ge[h], cx[h * Cp + D + lane], part);
      dqe[h] = 0.f;
      t[h] = part;
      dsb[h] = dc[h * Cp + C];          // d loss / d (Σ_j a'_jh): the gradient of the context's extra column
    }
    // delta_h = sum_j a_jh * da_jh = dctx_h . ctx_h + d(Σa')_h * (Σa')_h; interleaved butterflies
    pfo_wave_sum_scalar_n<H>(t);
#pragma unroll
    for (int h = 0; h < H; ++h) t[h] = fmaf(dsb[h], cx[h * Cp + C], t[h]);

    const unsigned keep = attn_keep_for(a, a.offset + (a.offset_dev ? *a.offset_dev : 0ull), n, lane);
    float my_a[H];
#pragma unroll
    for (int h = 0; h < H; ++h) my_a[h] = inK ? a.attw[(n * H + h) * K + lane] : 0.f;

    unsigned long long vm = valid;
    while (vm) {
      int js[KC_BWD];
#pragma unroll
      for (int c = 0; c < KC_BWD; ++c) {
        js[c] = vm ? (__ffsll((long long)vm) - 1) : -1;
        vm &= vm - 1ull;
      }
      float kn[KC_BWD][NR], kt[KC_BWD][NR], ks[KC_BWD][NR], ke[KC_BWD], dtv[KC_BWD];
      int rows[KC_BWD];
#pragma unroll
      for (int c = 0; c < KC_BWD; ++c) {
        const int j = js[c] < 0 ? 0 : js[c];
        rows[c] = rl_i(my_row, j);
        const float* src = a.nbr_tab + (int64_t)rows[c] * a.nbr_ld;
        const int e = rl_i(my_e, j);
        dtv[c] = rl_f(my_dt, j);
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int cc = lane + 64 * r;
          kn[c][r] = (js[c] >= 0 && (r < NR - 1 || cc < D)) ? src[cc] : 0.f;
        }
        ke[c] = (js[c] >= 0 && lane < Ef) ? a.edge_feat[(uint32_t)e * (uint32_t)Ef + (uint32_t)lane] : 0.f;
      }
      float part[KC_BWD][H];
#pragma unroll
      for (int c = 0; c < KC_BWD; ++c) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int cc = lane + 64 * r;
          float sv, cv;
          pfo_sincosf(pfo_time_arg(dtv[c], tw[r], tb[r]), sv, cv);
          const bool on = js[c] >= 0 && (r < NR - 1 || cc < D);     // select, not a branch (only the last r can be off)
          kt[c][r] = on ? cv : 0.f;
          ks[c][r] = on ? sv : 0.f;
        }
#pragma unroll
        for (int h = 0; h < H; ++h) {
          float pp = ke[c] * ge[h];
#pragma unroll
          for (int r = 0; r < NR; ++r) pp = fmaf(kn[c][r], gn[h][r], fmaf(kt[c][r], gt[h][r], pp));
          part[c][h] = pp;
        }
      }
#pragma unroll
      for (int c = 0; c < KC_BWD; ++c)
#pragma unroll
        for (int h = 0; h < H; ++h) part[c][h] = pfo_wave_sum_scalar(part[c][h]);
#pragma unroll
      for (int c = 0; c < KC_BWD; ++c) {
        if (js[c] < 0) continue;
        const unsigned kb = (unsigned)rl_i((int)keep, js[c]);
        float cA[H], cB[H];
#pragma unroll
        for (int h = 0; h < H; ++h) {
          const float ks_h = ((kb >> h) & 1u) ? keep_scale : 0.f;
          const float da = (part[c][h] + dsb[h]) * ks_h;               // d loss / d a_jh (through dropout)
          const float aj = rl_f(my_a[h], js[c]);
          const float dscore = aj * (da - t[h]);                       // softmax backward
          cA[h] = aj * ks_h;                                           // a'_jh multiplies dctx_h
          cB[h] = dscore * a.scale;                                    // multiplies qk_h
#pragma unroll
          for (int r = 0; r < NR; ++r) {
            dqn[h][r] = fmaf(cB[h], kn[c][r], dqn[h][r]);
            dqt[h][r] = fmaf(cB[h], kt[c][r], dqt[h][r]);
          }
          dqe[h] = fmaf(cB[h], ke[c], dqe[h]);
        }
        float* dst = (DMODE == 1 || DMODE == 2) ? d_nbr_x + (int64_t)rows[c] * a.d_nbr_ld : nullptr;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int cc = lane + 64 * r;
          float dkn = 0.f, dkt = 0.f;
#pragma unroll
          for (int h = 0; h < H; ++h) {
            dkn = fmaf(cA[h], gn[h][r], fmaf(cB[h], qn[h][r], dkn));
            dkt = fmaf(cA[h], gt[h][r], fmaf(cB[h], qt[h][r], dkt));
          }
          if (r < NR - 1 || cc < D) {                    // 64 * (NR - 1) < D: only the last r needs the lane test
            if (DMODE == 2) dst[cc] = (a.nbr_relu && !(kn[c][r] > 0.f)) ? 0.f : dkn;   // the row is a ReLU output of the layer below
            else if (DMODE == 1) atomicAdd(dst + cc, dkn);
            else if (DMODE == 3) det_add(a.d_nbr, (int64_t)rows[c] * a.d_nbr_ld + cc, dkn);
          }
          const float gsin = -ks[c][r] * dkt;            // d/d(arg) cos(arg) = -sin(arg); ks = 0 on lanes beyond D
          dw[r] += (double)gsin * (double)dtv[c];
          db[r] += (double)gsin;
        }
      }
    }
#pragma unroll
    for (int h = 0; h < H; ++h) {
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int c = lane + 64 * r;
        if (c < D) {
          dqk_out[h * Cp + c] = dqn[h][r];
          dqk_out[h * Cp + D + Ef + c] = dqt[h][r];
        }
      }
      if (lane < Ef) dqk_out[h * Cp + D + lane] = dqe[h];
      if (lane < Cp - C) dqk_out[h * Cp + C + lane] = 0.f;      // padding columns feed GEMMs: keep them finite
    }
  }
  // time-encoder partials: fold the four wavefronts, one slab row per workgroup (deterministic)
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    s_red[wave][0][lane + 64 * r] = dw[r];
    s_red[wave][1][lane + 64 * r] = db[r];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < 2 * D; c += 256) {
    const int which = c / D, cc = c - which * D;
    const double v = s_red[0][which][cc] + s_red[1][which][cc] + s_red[2][which][cc] + s_red[3][which][cc];
    // fp64 atomics into one of ATTN_TIME_BINS accumulator rows (all layers of a step share them; folded once at the end);
    // deterministic mode: this workgroup's own slab row (folded in row order)
    if (a.det) a.dtime_slab[(int64_t)blockIdx.x * 2 * D + c] = v;     // (once per workgroup: a run-time test costs nothing here)
    else atomicAdd(&a.dtime_part[(int64_t)(blockIdx.x & (ATTN_TIME_BINS - 1)) * 2 * D + c], v);
  }
}

// ---------------------------------------------------------------------------------------------
// KEY RING for the per-instance backward (round 6): the form above gathers a pair of keys into registers and uses them at once -
// one exposed round trip per pair, ten per instance - and its predicated first-level loads queue as dependent round trips
// (ISA notes at attn_fwd_ring_kernel).  Here, as in the ring forward: every first-level load clamped and in one batch, one
// LDS-DMA per key into a wavefront-private ring BWD_RING - 2 keys ahead of the pair being differentiated, [node | edge] columns
// as one vector on every side (key slot, qk' row, d ctx' row, d qk' row), counted vmcnt.  DMODE 0 (no key-side gradients:
// layer 1 without memory - C5) and 2 (plain stores: layers >= 2); the atomic forms keep the register kernel (layer 1 with
// memory takes the run-merged kernel anyway).  Same arithmetic per element as attn_bwd_body.
constexpr int BWD_RING = 4;
template <int NR, int H, int DMODE>
__device__ __forceinline__ void attn_bwd_ring_body(const AttnDev& a) {
  static_assert(DMODE == 0 || DMODE == 2, "ring form: no key-side gradients, or plain stores");
  constexpr int SLOTF = NR * 64, RP = BWD_RING / 2;
  __shared__ double s_red[4][2][NR * 64];
  __shared__ __align__(16) float s_ring[4][BWD_RING][SLOTF];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int D = a.D, Ef = a.Ef, K = a.K, DE = D + Ef, C = 2 * D + Ef, Cp = a.Cp;
  const bool direct = (a.nbr_row == nullptr);
  float tw[NR], tb[NR];
  double dw[NR], db[NR];     // sums of terms scaled by dt ~ 1e7 with heavy cancellation: accumulate in fp64
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int c = min(lane + 64 * r, D - 1);
    const float w = a.tw[c], b = a.tb[c];
    tw[r] = lane + 64 * r < D ? w : 0.f;
    tb[r] = lane + 64 * r < D ? b : 0.f;
    dw[r] = 0.0; db[r] = 0.0;
  }
  float* const ring = &s_ring[wave][0][0];
  if (lane + 64 * (NR - 1) >= DE)
#pragma unroll
    for (int s = 0; s < BWD_RING; ++s) ring[s * SLOTF + lane + 64 * (NR - 1)] = 0.f;     // (columns no DMA writes read as zero)
  const float keep_scale = a.dropout_p > 0.f ? 1.f / (1.f - a.dropout_p) : 1.f;
  const uint64_t rng_off = a.offset + (a.offset_dev ? *a.offset_dev : 0ull);
  typedef __attribute__((address_space(1))) const void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  const int D4 = D >> 2, DE4 = DE >> 2;
  const bool is_node = lane < D4;
  const uint64_t base_l = (is_node ? (uint64_t)(uintptr_t)a.nbr_tab : (uint64_t)(uintptr_t)a.edge_feat) + (uint64_t)((is_node ? lane : lane - D4) * 16);
  const uint32_t mul_l = is_node ? (uint32_t)a.nbr_ld * 4u : (uint32_t)Ef * 4u;
  const uint32_t node_mask = is_node ? 0xFFFFFFFFu : 0u;
  const bool inK = lane < K;

  for (int64_t n = (int64_t)blockIdx.x * 4 + wave; n < a.N; n += (int64_t)gridDim.x * 4) {
    float* dqk_out = a.dQK + n * H * Cp;
    const int64_t slot0 = n * K;
    // ---- first-level loads, clamped, one batch
    const int64_t si = slot0 + min(lane, K - 1);
    const int id_r = a.nbr_ids[si];
    const int row_l = (direct ? a.nbr_ids : a.nbr_row)[si];
    const int e_r = a.eidx[si];
    const float dt_r = a.dt[si];
    const int qrow_l = (a.qk_row ? a.qk_row : a.nbr_ids)[n];
    float a_r[H];
#pragma unroll
    for (int h = 0; h < H; ++h) a_r[h] = a.attw[(n * H + h) * K + min(lane, K - 1)];
    int my_id = inK ? id_r : 0, my_row = inK ? (direct ? (int)(a.nbr_row_base + si) : row_l) : 0, my_e = inK ? e_r : 0;
    float my_dt = inK ? dt_r : 0.f;
    float my_a[H];
#pragma unroll
    for (int h = 0; h < H; ++h) my_a[h] = inK ? a_r[h] : 0.f;
    const int qrow = a.qk_row ? qrow_l : (int)n;
    const unsigned long long valid = __ballot(inK && my_id != 0);
    if (DMODE == 2) {
      // padded slots own a gradient row too (the buffer is reused every step): zero it
      unsigned long long im = ~valid & (K >= 64 ? ~0ull : ((1ull << K) - 1ull));
      while (im) {
        const int j = __ffsll((long long)im) - 1;
        im &= im - 1ull;
        float* dst = a.d_nbr + (a.nbr_row_base + slot0 + j) * a.d_nbr_ld;
        for (int c = lane; c < D; c += 64) dst[c] = 0.f;
      }
    }
    if (valid == 0ull) {
      for (int c = lane; c < H * Cp; c += 64) dqk_out[c] = 0.f;
      continue;
    }
    // ---- second level: the instance's qk', d ctx' and ctx' rows (register-bound, clamped, in front of the DMAs)
    float q1[H][NR], qt[H][NR], g1[H][NR], gt[H][NR], t[H], dsb[H];
    {
      const float* qk = a.QK + (int64_t)qrow * a.qk_ld;
      const float* dc = a.dctx + n * H * Cp;
      const float* cx = a.ctx + n * H * Cp;
      float c1[H][NR], ct[H][NR], cs[H];
#pragma unroll
      for (int h = 0; h < H; ++h) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int k1 = min(lane + 64 * r, DE - 1), kt_ = min(lane + 64 * r, D - 1);
          q1[h][r] = qk[h * Cp + k1]; qt[h][r] = qk[h * Cp + DE + kt_];
          g1[h][r] = dc[h * Cp + k1]; gt[h][r] = dc[h * Cp + DE + kt_];
          c1[h][r] = cx[h * Cp + k1]; ct[h][r] = cx[h * Cp + DE + kt_];
        }
        dsb[h] = dc[h * Cp + C];          // d loss / d (sum_j a'_jh): the gradient of the context's extra column
        cs[h] = cx[h * Cp + C];
      }
#pragma unroll
      for (int h = 0; h < H; ++h) {
        float part = 0.f;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int c = lane + 64 * r;
          if (!(c < DE)) { q1[h][r] = 0.f; g1[h][r] = 0.f; c1[h][r] = 0.f; }
          if (!(c < D)) { qt[h][r] = 0.f; gt[h][r] = 0.f; ct[h][r] = 0.f; }
          part = fmaf(g1[h][r], c1[h][r], fmaf(gt[h][r], ct[h][r], part));
        }
        t[h] = part;
      }
      // delta_h = sum_j a_jh da_jh = d ctx'_h . ctx'_h + d(sum a')_h (sum a')_h
      pfo_wave_sum_scalar_n<H>(t);
#pragma unroll
      for (int h = 0; h < H; ++h) t[h] = fmaf(dsb[h], cs[h], t[h]);
    }
    const unsigned keep = attn_keep_for(a, rng_off, n, lane);
    // (every register-bound value is pinned in front of the first DMA: the compiler's wait for it must not sit behind one)
    asm volatile("" : "+v"(my_row), "+v"(my_e), "+v"(my_dt), "+v"(my_id));
#pragma unroll
    for (int h = 0; h < H; ++h) { asm volatile("" : "+v"(my_a[h]), "+v"(t[h]), "+v"(dsb[h])); }
    unsigned kp = keep;
    asm volatile("" : "+v"(kp));
    // ---- the ring: pair p = valid keys 2p, 2p + 1
    unsigned long long vm = valid;
    const int n_pairs = (__popcll(valid) + 1) >> 1;
    int issued = 0;
    auto issue_pair = [&]() {
      int j0 = __ffsll((long long)vm) - 1;
      vm &= vm - 1ull;
      int j1 = vm ? (__ffsll((long long)vm) - 1) : j0;
      vm &= vm - 1ull;
      const int sl = (2 * issued) % BWD_RING;
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
    float dq1[H][NR], dqt[H][NR];
#pragma unroll
    for (int h = 0; h < H; ++h)
#pragma unroll
      for (int r = 0; r < NR; ++r) { dq1[h][r] = 0.f; dqt[h][r] = 0.f; }
    unsigned long long wm = valid;
    for (int p = 0; p < n_pairs; ++p) {
      int js[2];
      js[0] = __ffsll((long long)wm) - 1;
      wm &= wm - 1ull;
      js[1] = wm ? (__ffsll((long long)wm) - 1) : -1;
      wm &= wm - 1ull;
      const bool more = p + RP < n_pairs;
      if (more) pfo_wait_vm<2 * (RP - 1)>(); else pfo_wait_vm<0>();
      const float* sl = ring + ((2 * p) % BWD_RING) * SLOTF;
      float kn[2][NR], kt[2][NR], ks[2][NR], dtv[2];
      int rows[2];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int j = js[c] < 0 ? js[0] : js[c];
        rows[c] = rl_i(my_row, j);
        dtv[c] = rl_f(my_dt, j);
#pragma unroll
        for (int r = 0; r < NR; ++r) kn[c][r] = sl[c * SLOTF + lane + 64 * r];
      }
      float part[2 * H];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          float sv, cv;
          pfo_sincosf(pfo_time_arg(dtv[c], tw[r], tb[r]), sv, cv);
          const bool on = r < NR - 1 || lane + 64 * r < D;
          kt[c][r] = on ? cv : 0.f;
          ks[c][r] = on ? sv : 0.f;
        }
#pragma unroll
        for (int h = 0; h < H; ++h) {
          float pp = 0.f;
#pragma unroll
          for (int r = 0; r < NR; ++r) pp = fmaf(kn[c][r], g1[h][r], fmaf(kt[c][r], gt[h][r], pp));
          part[c * H + h] = pp;
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // the slots' values sit in registers: the pair RP ahead starts its trip
      if (more) issue_pair();
      pfo_wave_sum_scalar_n<2 * H>(part);
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        if (js[c] < 0) continue;
        const unsigned kb = (unsigned)rl_i((int)kp, js[c]);
        float cA[H], cB[H];
#pragma unroll
        for (int h = 0; h < H; ++h) {
          const float ks_h = ((kb >> h) & 1u) ? keep_scale : 0.f;
          const float da = (part[c * H + h] + dsb[h]) * ks_h;            // d loss / d a_jh (through dropout)
          const float aj = rl_f(my_a[h], js[c]);
          const float dscore = aj * (da - t[h]);                         // softmax backward
          cA[h] = aj * ks_h;                                             // a'_jh multiplies d ctx'_h
          cB[h] = dscore * a.scale;                                      // multiplies qk'_h
#pragma unroll
          for (int r = 0; r < NR; ++r) {
            dq1[h][r] = fmaf(cB[h], kn[c][r], dq1[h][r]);
            dqt[h][r] = fmaf(cB[h], kt[c][r], dqt[h][r]);
          }
        }
        float* dst = (DMODE == 2) ? a.d_nbr + (int64_t)rows[c] * a.d_nbr_ld : nullptr;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int cc = lane + 64 * r;
          float dkn = 0.f, dkt = 0.f;
#pragma unroll
          for (int h = 0; h < H; ++h) {
            dkn = fmaf(cA[h], g1[h][r], fmaf(cB[h], q1[h][r], dkn));
            dkt = fmaf(cA[h], gt[h][r], fmaf(cB[h], qt[h][r], dkt));
          }
          if (DMODE == 2 && cc < D) dst[cc] = (a.nbr_relu && !(kn[c][r] > 0.f)) ? 0.f : dkn;   // the row is a ReLU output of the layer below
          const float gsin = -ks[c][r] * dkt;            // d/d(arg) cos(arg) = -sin(arg); ks = 0 on lanes beyond D
          dw[r] += (double)gsin * (double)dtv[c];
          db[r] += (double)gsin;
        }
      }
    }
#pragma unroll
    for (int h = 0; h < H; ++h) {
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int c = lane + 64 * r;
        if (c < DE) dqk_out[h * Cp + c] = dq1[h][r];
        if (c < D) dqk_out[h * Cp + DE + c] = dqt[h][r];
      }
      if (lane < Cp - C) dqk_out[h * Cp + C + lane] = 0.f;      // padding columns feed GEMMs: keep them finite
    }
    // (the stores above are drained before the next instance's DMAs by the compiler: a store round trip per instance, behind ~20 keys of arithmetic)
  }
  // time-encoder partials: fold the four wavefronts, one slab row per workgroup (deterministic)
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    s_red[wave][0][lane + 64 * r] = dw[r];
    s_red[wave][1][lane + 64 * r] = db[r];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < 2 * D; c += 256) {
    const int which = c / D, cc = c - which * D;
    const double v = s_red[0][which][cc] + s_red[1][which][cc] + s_red[2][which][cc] + s_red[3][which][cc];
    if (a.det) a.dtime_slab[(int64_t)blockIdx.x * 2 * D + c] = v;
    else atomicAdd(&a.dtime_part[(int64_t)(blockIdx.x & (ATTN_TIME_BINS - 1)) * 2 * D + c], v);
  }
}

// minimum wavefronts per SIMD the register allocation must allow: 3 where the kernel fits 168 VGPRs without spilling
#define BWD_WAVES(NR, H, DMODE) (((H) <= 2 && (NR) <= 3) ? ((DMODE) == 1 ? 2 : 3) : (((H) == 4 && (NR) == 4) ? 1 : 2))
template <int NR, int H> __global__ __launch_bounds__(256, BWD_WAVES(NR, H, 0)) void attn_bwd_ring_kernel_none(const AttnDev a) { attn_bwd_ring_body<NR, H, 0>(a); }
template <int NR, int H> __global__ __launch_bounds__(256, BWD_WAVES(NR, H, 2)) void attn_bwd_ring_kernel_direct(const AttnDev a) { attn_bwd_ring_body<NR, H, 2>(a); }
template <int NR, int H> __global__ __launch_bounds__(256, BWD_WAVES(NR, H, 0)) void attn_bwd_kernel_none(const AttnDev a) { attn_bwd_body<NR, H, 0>(a); }
template <int NR, int H> __global__ __launch_bounds__(256, BWD_WAVES(NR, H, 1)) void attn_bwd_kernel(const AttnDev a) { attn_bwd_body<NR, H, 1>(a); }
template <int NR, int H> __global__ __launch_bounds__(256, BWD_WAVES(NR, H, 2)) void attn_bwd_kernel_direct(const AttnDev a) { attn_bwd_body<NR, H, 2>(a); }
template <int NR, int H> __global__ __launch_bounds__(256, BWD_WAVES(NR, H, 1)) void attn_bwd_kernel_det(const AttnDev a) { attn_bwd_body<NR, H, 3>(a); }

int attn_bwd_run(int form, dim3 grid, dim3 block, const AttnDev& d, hipStream_t stream) {
  bool done;
  if (form == PFO_ATTN_FORM_BWD_RING_NONE) done = attn_for_shape<ATTN_RING_MAX_NRH>(d.D, d.H, [&](auto nr, auto h) { PFO_KLAUNCH((attn_bwd_ring_kernel_none<nr, h>), grid, block, 0, stream, d); });
  else if (form == PFO_ATTN_FORM_BWD_RING_DIRECT) done = attn_for_shape<ATTN_RING_MAX_NRH>(d.D, d.H, [&](auto nr, auto h) { PFO_KLAUNCH((attn_bwd_ring_kernel_direct<nr, h>), grid, block, 0, stream, d); });
  else if (form == PFO_ATTN_FORM_BWD_NONE) done = attn_for_shape<ATTN_MAX_NRH>(d.D, d.H, [&](auto nr, auto h) { PFO_KLAUNCH((attn_bwd_kernel_none<nr, h>), grid, block, 0, stream, d); });
  else if (form == PFO_ATTN_FORM_BWD_DET) done = attn_for_shape<ATTN_MAX_NRH>(d.D, d.H, [&](auto nr, auto h) { PFO_KLAUNCH((attn_bwd_kernel_det<nr, h>), grid, block, 0, stream, d); });
  else if (form == PFO_ATTN_FORM_BWD_ATOMIC) done = attn_for_shape<ATTN_MAX_NRH>(d.D, d.H, [&](auto nr, auto h) { PFO_KLAUNCH((attn_bwd_kernel<nr, h>), grid, block, 0, stream, d); });
  else done = attn_for_shape<ATTN_MAX_NRH>(d.D, d.H, [&](auto nr, auto h) { PFO_KLAUNCH((attn_bwd_kernel_direct<nr, h>), grid, block, 0, stream, d); });
  PFO_REQUIRE(done, "unsupported (D, H) combination");
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}
