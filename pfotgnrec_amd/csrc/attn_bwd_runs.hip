// The run-merged layer-1 attention backward with its shader-clock pair (RUN_CHUNK and RUN_CPW, which attn.hip sizes the grid
// by, are in attn_dev.hpp).
#include "attn_dev.hpp"

// ---------------------------------------------------------------------------------------------
// Layer-1 backward with SHIFT MERGING.  The level-0 gradient scatter is bound by the float-atomic rate of the part (~1.3 TB/s of
// added bytes chip-wide, MI355X_MICROARCH.md: one 256-byte wave instruction per ~50 ns per CU); everything else in this kernel
// hides behind it.  Instances arrive ordered by (touched-table row, entries of the row's history before the instance's time) -
// memory.hpp pfo_seg_build_launch - so consecutive members of a row walk its history forwards, and under most-recent sampling
// slot j of an instance holds history entry cnt - K + j: the neighbour lists of two instances of one node are SHIFTS of each
// other by the difference of their counts (identical when the counts are equal - every ~4 instances of a user in a batch;
// shifted by one or two entries for the instances of an item, whose history grows inside the batch window).
// One wavefront (a 64-thread workgroup) walks a chunk of RUN_CHUNK consecutive members.  Lane q stands for history entry
// cnt0 - K + q of the group's first instance; an instance whose count is cnt0 + d puts its slot j on lane j + d.  The key-side
// gradient rows of a group leave as ONE set of float atomics, one row per distinct history entry, when the row, the lane range
// (K + d <= 64) or the chunk ends.  Round 2 merged only identical lists (d = 0): at C2 that left the ~12 k item instances, 55 %
// of the atomic instructions, unmerged.
//
// The rows are not accumulated while the instances are walked.  The gradient of a neighbour row summed over a group is
//     sum_i sum_h ( cA_ih * g_ih  +  cB_ih * q_h )        g_ih = d ctx'_h (node part) of instance i,  q_h = the node's query
// with wave-uniform scalars cA (post-dropout weight) and cB (d score * scale), and q_h is the same for every instance of the
// node.  So the walk only keeps the SCALARS - per instance and slot cA (LDS), per lane the running sum of cB (a register) - and
// the rows are formed once per group from the re-read g rows (just used: cache hits).
constexpr int KC_RUNS = 2;      // keys in flight per wavefront
#define RUNS_WAVES(NR, H) ((NR) * (H) <= 6 ? 3 : 2)
// shader-clock pair 1 of pfo_shader_clock; the device symbol and its reader share this file
__device__ unsigned long long g_attn_bwd_runs_clock[2];
int attn_bwd_runs_clock_read(double* out, int reset) { return attn_clock_pair_read(HIP_SYMBOL(g_attn_bwd_runs_clock), out, reset); }
// MEMBER STAGING (round 5).  In-kernel stamps (round 5, profiles/) showed where a wavefront's life
// went: 47 % in the member set-up, 32 % walking the 20 keys, 12 % in the flush - the set-up is a chain of dependent round trips
// (members[m] -> qk_row[n] / run_cnt[n] -> the query row; then d ctx' and ctx', streamed from HBM exactly once by this kernel,
// ~9 us per member against ~6 us for the walk), paid once per member with three wavefronts per SIMD to hide it.  Now:
//  * a chunk prologue resolves the indirections of ALL its members at once (one lane per member: two dependent loads per chunk);
//  * the rows of member i+1 (d ctx', ctx', the node's query row: 3 x H Cp floats) and its per-slot metadata (neighbour ids, table
//    rows, edge ids, dt, the attention weights: (4 + H) x K words) travel by LDS-DMA (global_load_lds: no registers, no wait)
//    into a wavefront-private staging image while member i is walked; the set-up of member i+1 reads LDS.  EXEC masks the
//    lanes behind a row's end (tools/probes/lds_dma_mask.hip: masked lanes write nothing);
//  * the flush takes the run's member ids from the prologue's register instead of re-loading members[].
// The r4 one-dword-per-line touch of the next rows (-2 %, +36 % fetched bytes) is gone.
// How a wavefront spends its cycles (round 3; measured against the round-2 loop, 357 vs 363 us at equal atomics - the atomic
// rate, not the issue rate, bounds this kernel):
//  * the gathers of key chunk c+1 are issued before chunk c is scored (two register sets used alternately, as in the forward);
//  * no exec-mask region and no select in the key loop: gathers read clamped addresses (the last 64-column group re-reads
//    column D-1, the edge lanes column Ef-1) instead of being predicated, and the lanes they feed carry zero query / gradient
//    values or are never stored; the time-encoder parameters are zero beyond D, so the encodings there are cos(0), sin(0);
//  * the "argument too large for the fp32 range reduction" test is taken once per INSTANCE from max|dt| * max|w| + max|b|
//    (wave-uniform), not per chunk on every argument;
//  * the per-key softmax-backward scalars of a chunk are reduced together (one interleaved DPP tree for KC*H sums), the running
//    sum of cB per key lives in a register (select on lane == key) instead of an LDS read-modify-write.
template <int NR, int H, bool DET>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(RUNS_WAVES(NR, H)))) void attn_bwd_runs_kernel(const AttnDev a) {
  __shared__ float s_tw[NR * 64], s_tb[NR * 64];
  __shared__ float s_cA[RUN_CHUNK][H][64];     // [instance of the group][head][slot]: cA of that key; zero where the slot is empty
  __shared__ int s_delta[RUN_CHUNK];            // [instance of the group]: its shift (count - the group's first count)
  __shared__ int s_ch[3][RUN_CPW * RUN_CHUNK];  // the wavefront's members: instance id, query row, history count (prologue)
  // staging image (dynamic LDS, sized by the launcher: pfo_attn_runs_lds_bytes): [d ctx' row | ctx' row | query row | metadata]
  extern __shared__ __align__(16) unsigned char s_stage[];
  const int lane = threadIdx.x;
  const int D = a.D, Ef = a.Ef, K = a.K, C = 2 * D + Ef, Cp = a.Cp;
  const bool clk_on = blockIdx.x == 0;
  PfoClockStamp clk;
  if (clk_on) clk = pfo_clock_begin();
  // Two chains of dependent loads open a wavefront's life: (A) *n_rows -> seg_ptr[.] = the members' count M, (B) the
  // wavefront's member ids -> their query rows / history counts.  (B) is issued speculatively - clamped indices, no dependence
  // on M - so the two chains overlap instead of queueing (a wavefront lives ~35 us: every round trip is 3-4 % of it).
  constexpr int UM = RUN_CPW * RUN_CHUNK;                          // members per wavefront
  const int G8 = 8 * a.xcd_g;
  auto unit_of = [&](int blk) {
    if (G8 <= 0) return blk;
    const int grp = blk / G8, r = blk - grp * G8;
    return grp * G8 + (r & 7) * a.xcd_g + (r >> 3);
  };
  auto spec_member = [&](int unit) { return a.members[min(unit * UM + min(lane, UM - 1), a.N - 1)]; };
  int sp_raw = spec_member(unit_of((int)blockIdx.x));
  const int nr_rows = *a.n_rows;
  float wmax = 0.f, bmax = 0.f;
  {
    // (clamped addresses, not predicated loads: the six loads leave together - predicated, each 64-column group waited for
    // its own round trip at the head of every wavefront's life)
    float wv[NR], bv[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) { const int cc = min(lane + 64 * r, D - 1); wv[r] = a.tw[cc]; bv[r] = a.tb[cc]; }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int c = lane + 64 * r;
      const float w = c < D ? wv[r] : 0.f, b = c < D ? bv[r] : 0.f;
      s_tw[c] = w; s_tb[c] = b;
      wmax = fmaxf(wmax, fabsf(w)); bmax = fmaxf(bmax, fabsf(b));
    }
  }
  sp_raw = min(max(sp_raw, 0), a.N - 1);                           // (behind the members' count the list holds anything)
  int sp_slot = a.qk_row[sp_raw], sp_cnt = a.run_cnt[sp_raw];
  const int M = a.seg_ptr[nr_rows];                                // members = instances that sit on a real node
  const int n_chunks = (M + RUN_CHUNK - 1) / RUN_CHUNK;
  wmax = pfo_wave_max(wmax); bmax = pfo_wave_max(bmax);
  // clamped column of this lane in each 64-column group, and the edge column
  int colr[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) colr[r] = min(lane + 64 * r, D - 1);
  const int cole = min(lane, max(Ef, 1) - 1);
  const float keep_scale = a.dropout_p > 0.f ? 1.f / (1.f - a.dropout_p) : 1.f;
  float* const d_nbr_x = a.d_nbr + (int64_t)(__builtin_amdgcn_s_getreg(6164) & (a.d_nbr_nrep - 1)) * a.d_nbr_rep;
  const uint64_t rng_off = a.offset + (a.offset_dev ? *a.offset_dev : 0ull);
  const float* const nbr_tab = a.nbr_tab;
  const float* const edge_feat = a.edge_feat;
  const uint32_t nbr_ld = (uint32_t)a.nbr_ld;
  // the staging image and the LDS-DMA that fills it (one member at a time; the issuing wavefront's vmcnt covers it)
  typedef __attribute__((address_space(1))) const void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  const uint32_t row_bytes = (uint32_t)(H * Cp) * 4u;             // a multiple of 16 (Cp is a multiple of 4)
  const float* const st_dc = reinterpret_cast<const float*>(s_stage);
  const float* const st_cx = reinterpret_cast<const float*>(s_stage + row_bytes);
  const float* const st_qk = reinterpret_cast<const float*>(s_stage + 2 * row_bytes);
  unsigned char* const st_meta = s_stage + 3 * row_bytes;        // (4 + H) arrays of K words: ids, table rows, edge ids, dt, weights
  const bool inject = a.keep_inject != nullptr && a.dropout_p > 0.f;
  auto stage = [&](int64_t n, int slot) {
    const char* g_dc = reinterpret_cast<const char*>(a.dctx + n * H * Cp);
    const char* g_cx = reinterpret_cast<const char*>(a.ctx + n * H * Cp);
    const char* g_qk = reinterpret_cast<const char*>(a.QK + (int64_t)slot * a.qk_ld);
    // (the lane offset is made opaque: hoisted out of the member loop, the per-lane addresses of nine loads would be kept alive
    // as 64-bit register pairs across the key walk - the kernel sits at its register limit, they went to scratch)
    uint32_t lo = (uint32_t)lane * 4u;
    asm volatile("" : "+v"(lo));
    for (uint32_t k = 0; k * 1024u < row_bytes; ++k) {
      const uint32_t off = k * 1024u + lo * 4u;
      if (off < row_bytes) {                                     // lanes behind the row's end stay off: they write nothing
        __builtin_amdgcn_global_load_lds((gptr_t)(g_dc + off), (lptr_t)(s_stage + k * 1024u), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((gptr_t)(g_cx + off), (lptr_t)(s_stage + row_bytes + k * 1024u), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((gptr_t)(g_qk + off), (lptr_t)(s_stage + 2 * row_bytes + k * 1024u), 16, 0, 0);
      }
    }
    if (lane < K) {
      // wave-uniform row starts + ONE 32-bit lane offset (the scalar-base form of the load: no per-lane 64-bit pointers to keep)
      const uint32_t kb = (uint32_t)K * 4u;
      const int64_t s0 = n * K;
      __builtin_amdgcn_global_load_lds((gptr_t)(reinterpret_cast<const char*>(a.nbr_ids + s0) + lo), (lptr_t)(st_meta), 4, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr_t)(reinterpret_cast<const char*>(a.nbr_row + s0) + lo), (lptr_t)(st_meta + kb), 4, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr_t)(reinterpret_cast<const char*>(a.eidx + s0) + lo), (lptr_t)(st_meta + 2 * kb), 4, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr_t)(reinterpret_cast<const char*>(a.dt + s0) + lo), (lptr_t)(st_meta + 3 * kb), 4, 0, 0);
#pragma unroll
      for (int h = 0; h < H; ++h)
        __builtin_amdgcn_global_load_lds((gptr_t)(reinterpret_cast<const char*>(a.attw + (n * H + h) * K) + lo), (lptr_t)(st_meta + (4 + h) * kb), 4, 0, 0);
      // injected dropout decisions (parity tests) ride in the image too, one byte per slot (a dword of LDS each): a register-bound load of them in
      // the member's set-up put the compiler's s_waitcnt vmcnt(0) for it - taken whether or not the load ran - right behind
      // these DMAs: every member waited out the staging round trip it was meant to walk beside
      if (inject) __builtin_amdgcn_global_load_lds((gptr_t)(reinterpret_cast<const char*>(a.keep_inject + s0) + (lo >> 2)), (lptr_t)(st_meta + (4 + H) * kb), 1, 0, 0);
    }
  };

  // Workgroups go to the XCDs round-robin by their id.  Consecutive chunks hold members of the same table row or of
  // neighbouring ones (the list is ordered by row): with xcd_g = G > 0 every XCD takes G consecutive chunks at a time (block b ->
  // chunk (b / 8G) 8G + (b mod 8) G + (b mod 8G) / 8), so the shifted neighbour lists of one node's members, its query row and
  // the rows its atomics land on stay in ONE L2 instead of being fetched by up to eight.
  // A wavefront takes a UNIT of RUN_CPW consecutive chunks.  The chunk stays the scope of a run (its rows leave at the chunk's
  // end at the latest) and of the time-encoder partial sums; the unit is the scope of the prologue and of the member staging.
  const int n_units = (n_chunks + RUN_CPW - 1) / RUN_CPW;
  const int n_walk = G8 > 0 ? (n_units + G8 - 1) / G8 * G8 : n_units;
  for (int blk = blockIdx.x; blk < n_walk; blk += gridDim.x) {
    const int unit = unit_of(blk);
    if (blk != (int)blockIdx.x) {                                  // (a capped grid only: later units load their prologue here)
      sp_raw = min(max(spec_member(unit), 0), a.N - 1);
      sp_slot = a.qk_row[sp_raw]; sp_cnt = a.run_cnt[sp_raw];
    }
    if (unit >= n_units) continue;
    // prologue: the members' instance ids, query rows and history counts, one lane per member, and the first member's rows
    // on their way
    const int u0 = unit * UM;
    const int u_end = min(M, u0 + UM);
    {
      const bool ch_on = lane < UM && u0 + lane < u_end;
      const int ch_n = ch_on ? sp_raw : 0;
      const int ch_slot = ch_on ? sp_slot : -1;
      const int ch_cnt = ch_on ? sp_cnt : 0;
      if (lane < UM) { s_ch[0][lane] = ch_n; s_ch[1][lane] = ch_slot; s_ch[2][lane] = ch_cnt; }   // (one wavefront: no barrier)
      if (u0 < u_end) stage(rl_i(ch_n, 0), rl_i(ch_slot, 0));
    }
    auto ch_get = [&](int which, int i) { return __builtin_amdgcn_readfirstlane(s_ch[which][i]); };
    for (int chunk = unit * RUN_CPW; chunk < min(n_chunks, (unit + 1) * RUN_CPW); ++chunk) {
    const int m0 = chunk * RUN_CHUNK;
    const int m_end = min(M, m0 + RUN_CHUNK);
    float dwc[NR], dbc[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) { dwc[r] = 0.f; dbc[r] = 0.f; }
    // the current group: lane q <-> history entry cnt0 - K + q of the node run_slot
    int run_slot = -1, run_cnt0 = 0, run_rows = 0, run_len = 0, run_first = 0;
    unsigned long long run_valid = 0ull;                           // lanes whose history entry exists and was seen
    // The query-side gradient rows [dqk' (node | edge | time)] of consecutive members that sit on ONE table row are summed
    // here, in registers, and stored once (row acc_m, flagged live): the per-row sum pass that follows (segsum) adds the
    // members of a row anyway, and a chunk of 4 members holds ~2.5 per row at C2 - less than half the rows are written / re-read
    float dqn[H][NR], dqt[H][NR], dqe[H];
    int acc_m = -1;
    auto acc_reset = [&]() {
#pragma unroll
      for (int h = 0; h < H; ++h) {
#pragma unroll
        for (int r = 0; r < NR; ++r) { dqn[h][r] = 0.f; dqt[h][r] = 0.f; }
        dqe[h] = 0.f;
      }
    };
    // (acc_store, flush and stage address their rows as a wave-uniform base + ONE 32-bit lane offset that is opaque to the
    // optimiser: hoisted out of the member loop, their per-lane 64-bit element offsets lived across the key walk - a dozen
    // register pairs at a kernel that sits on its register limit, i.e. scratch reloads in front of every store)
    auto acc_store = [&]() {
      if (acc_m >= 0) {
        char* out = reinterpret_cast<char*>(a.dQK + (int64_t)acc_m * H * Cp);      // row m, not n: the per-row sums then stream contiguous rows
        uint32_t lo = (uint32_t)lane * 4u;
        asm volatile("" : "+v"(lo));
#pragma unroll
        for (int h = 0; h < H; ++h) {
#pragma unroll
          for (int r = 0; r < NR; ++r) {
            if (lo < (uint32_t)(D - 64 * r) * 4u) {              // column lane + 64 r < D (64 r < D for every r < NR)
              *reinterpret_cast<float*>(out + (uint32_t)(h * Cp + 64 * r) * 4u + lo) = dqn[h][r];
              *reinterpret_cast<float*>(out + (uint32_t)(h * Cp + D + Ef + 64 * r) * 4u + lo) = dqt[h][r];
            }
          }
          if (lo < (uint32_t)Ef * 4u) *reinterpret_cast<float*>(out + (uint32_t)(h * Cp + D) * 4u + lo) = dqe[h];
          if (lo < (uint32_t)(Cp - C) * 4u) *reinterpret_cast<float*>(out + (uint32_t)(h * Cp + C) * 4u + lo) = 0.f;
        }
        if (lane == 0) a.dqk_live[acc_m] = 1;
      }
      acc_m = -1;
      acc_reset();
    };
    acc_reset();
    float sBr[H];                                                  // lane q: sum of cB over the group's instances that hold entry q
#pragma unroll
    for (int h = 0; h < H; ++h) sBr[h] = 0.f;
    auto flush = [&]() {                                           // the run's rows: one float atomic per element
      if (run_valid != 0ull && run_len > 0) {
        const char* qk = reinterpret_cast<const char*>(a.QK + (int64_t)run_slot * a.qk_ld);
        uint32_t lo = (uint32_t)lane * 4u;
        asm volatile("" : "+v"(lo));
        float qn[H][NR], g[RUN_CHUNK][H][NR];
#pragma unroll
        for (int h = 0; h < H; ++h)
#pragma unroll
          for (int r = 0; r < NR; ++r)
            qn[h][r] = lo < (uint32_t)(D - 64 * r) * 4u ? *reinterpret_cast<const float*>(qk + (uint32_t)(h * Cp + 64 * r) * 4u + lo) : 0.f;
        float cAr[RUN_CHUNK][H];                                   // lane q: cA of the slot instance i has on history entry q
#pragma unroll
        for (int i = 0; i < RUN_CHUNK; ++i) {
          const bool on = i < run_len;                             // wave-uniform
          const char* dc = reinterpret_cast<const char*>(a.dctx + (int64_t)ch_get(0, (on ? run_first + i : run_first) - u0) * H * Cp);
          const int sl = lane - (on ? s_delta[i] : 0);             // the instance's slot on this lane (may lie outside [0, K): zero)
#pragma unroll
          for (int h = 0; h < H; ++h) {
            cAr[i][h] = (on && sl >= 0) ? s_cA[i][h][sl < 0 ? 0 : sl] : 0.f;
#pragma unroll
            for (int r = 0; r < NR; ++r)
              g[i][h][r] = (on && lo < (uint32_t)(D - 64 * r) * 4u) ? *reinterpret_cast<const float*>(dc + (uint32_t)(h * Cp + 64 * r) * 4u + lo) : 0.f;
          }
        }
        unsigned long long vmask = run_valid;
        while (vmask) {
          const int j = __ffsll((long long)vmask) - 1;
          vmask &= vmask - 1ull;
          const int64_t drow = (int64_t)rl_i(run_rows, j) * a.d_nbr_ld;
          char* dst = reinterpret_cast<char*>(d_nbr_x + drow);
          float row[NR];
#pragma unroll
          for (int r = 0; r < NR; ++r) row[r] = 0.f;
#pragma unroll
          for (int h = 0; h < H; ++h) {
            const float sb = rl_f(sBr[h], j);
#pragma unroll
            for (int r = 0; r < NR; ++r) row[r] = fmaf(sb, qn[h][r], row[r]);
#pragma unroll
            for (int i = 0; i < RUN_CHUNK; ++i) {
              const float ca = rl_f(cAr[i][h], j);                 // 0 beyond the run's length
#pragma unroll
              for (int r = 0; r < NR; ++r) row[r] = fmaf(ca, g[i][h][r], row[r]);
            }
          }
#pragma unroll
          for (int r = 0; r < NR; ++r) {
            if (r < NR - 1 || lo < (uint32_t)(D - 64 * r) * 4u) {
              if (DET) det_add(a.d_nbr, drow + lane + 64 * r, row[r]); else atomicAdd(reinterpret_cast<float*>(dst + (uint32_t)(256 * r) + lo), row[r]);
            }
          }
        }
      }
#pragma unroll
      for (int h = 0; h < H; ++h) sBr[h] = 0.f;
      run_len = 0;
    };

    for (int m = m0; m < m_end; ++m) {
      const int64_t n = ch_get(0, m - u0);
      const int slot = ch_get(1, m - u0);
      const int cnt_n = ch_get(2, m - u0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this member's staging image has landed
      const bool inK = lane < K;
      const int* const mi = reinterpret_cast<const int*>(st_meta);
      const int my_id = inK ? mi[lane] : 0;
      const int my_row = inK ? mi[K + lane] : 0;
      const int my_e = inK ? mi[2 * K + lane] : 0;
      const float my_dt = inK ? __int_as_float(mi[3 * K + lane]) : 0.f;
      const unsigned long long valid = __ballot(inK && my_id != 0);
      int delta = cnt_n - run_cnt0;                              // members of a row arrive by ascending count
      if (slot != run_slot || delta < 0 || delta > 64 - K) {     // another node, or the lanes run out: the group's rows leave
        acc_store();                                             // (the query-side sums too: never live across a flush)
        flush();
        run_slot = slot; run_cnt0 = cnt_n; run_rows = 0; run_valid = 0ull;
        delta = 0;
      }
      {
        // this instance's slots move to lanes j + delta: row indices and validity join the group's
        const int rows_sh = __builtin_amdgcn_ds_bpermute((lane - delta) << 2, my_row);
        const unsigned long long vs = valid << delta;
        run_rows = ((vs >> lane) & 1ull) ? rows_sh : run_rows;
        run_valid |= vs;
      }
      if (lane == 0) a.dqk_live[m] = 0;                         // (set when this member's position receives a stored sum)
      if (valid == 0ull) {                                       // no neighbour: nothing to add to the row's sums
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (m + 1 < u_end) stage(ch_get(0, m + 1 - u0), ch_get(1, m + 1 - u0));
        continue;
      }
      acc_m = m;
      if (run_len == 0) run_first = m;                           // the group's instances with a neighbour are consecutive members
      const int run_i = run_len;                                 // (an instance without history has count 0: first of its row)
      run_len += 1;
      s_delta[run_i] = delta;
      float qt[H][NR], gn[H][NR], gt[H][NR], ge[H], tds[2 * H];
      float dsb[H], cxs[H], my_a[H];
#pragma unroll
      for (int h = 0; h < H; ++h) {
        float part = 0.f;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int c = lane + 64 * r;
          const bool ok = c < D;
          qt[h][r] = ok ? st_qk[h * Cp + D + Ef + c] : 0.f;
          gn[h][r] = ok ? st_dc[h * Cp + c] : 0.f;
          gt[h][r] = ok ? st_dc[h * Cp + D + Ef + c] : 0.f;
          if (ok) part = fmaf(gn[h][r], st_cx[h * Cp + c], fmaf(gt[h][r], st_cx[h * Cp + D + Ef + c], part));
        }
        ge[h] = lane < Ef ? st_dc[h * Cp + D + lane] : 0.f;
        if (lane < Ef) part = fmaf(ge[h], st_cx[h * Cp + D + lane], part);
        tds[h] = part;
        dsb[h] = st_dc[h * Cp + C];          // d loss / d (sum_j a'_jh): one address for the wavefront (an LDS broadcast)
        cxs[h] = st_cx[h * Cp + C];
        my_a[h] = inK ? __int_as_float(mi[(4 + h) * K + lane]) : 0.f;
      }
      // injected dropout decisions: read HERE, with the rest of the image, in front of the next member's staging (a sub-dword
      // LDS-DMA load writes one zero-extended DWORD per lane: the bytes sit at a stride of four)
      const unsigned keep_img = (inject && inK) ? ((unsigned)mi[(4 + H) * K + lane] & 0xFFu) : 0xFu;
      // the image is free again: the next member's rows start their trip here and land while this member is walked
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (m + 1 < u_end) stage(ch_get(0, m + 1 - u0), ch_get(1, m + 1 - u0));
      pfo_wave_sum_scalar_n<H>(reinterpret_cast<float(&)[H]>(tds));     // delta_h = dctx_h . ctx_h (+ the extra column below)
      float t[H];
#pragma unroll
      for (int h = 0; h < H; ++h) {
        dsb[h] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(dsb[h])));
        t[h] = fmaf(dsb[h], __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(cxs[h]))), tds[h]);
      }
      // Per slot, once per member: the dropout multiplier ks_jh (0 or 1 / (1 - p)) and with it cA_jh = a_jh ks_jh - the
      // coefficient of d ctx'_h in the key-side rows does not depend on the backward at all: it goes to the group's LDS table
      // here (one store per head) instead of from inside the key loop (compare + exec-masked store per key), and the loop reads
      // ks with one v_readlane per head instead of unpacking a bit mask (scalar and / compare / select + a vector select)
      float my_ks[H];
      {
        const unsigned keep = inject ? keep_img : attn_keep_bits(a.seed, rng_off, n, lane, a.dropout_p);
#pragma unroll
        for (int h = 0; h < H; ++h) {
          my_ks[h] = ((keep >> h) & 1u) ? keep_scale : 0.f;
          s_cA[run_i][h][lane] = ((valid >> lane) & 1ull) ? my_a[h] * my_ks[h] : 0.f;
        }
      }
      // one range test per instance: |fma(dt, w, b)| <= max|dt| max|w| + max|b| < 2e7 -> the fp32 reduction holds for every key
      const bool fast = fmaf(pfo_wave_max(fabsf(my_dt)), wmax, bmax) < 2.0e7f;

      auto walk = [&](auto fast_c) {
      constexpr bool FAST = decltype(fast_c)::value;
      unsigned long long vm = valid;
      int jsA[KC_RUNS], jsB[KC_RUNS];
      float knA[KC_RUNS][NR], keA[KC_RUNS], knB[KC_RUNS][NR], keB[KC_RUNS];
      auto pick = [&](int (&jj)[KC_RUNS]) {
#pragma unroll
        for (int c = 0; c < KC_RUNS; ++c) {
          jj[c] = vm ? (__ffsll((long long)vm) - 1) : -1;
          vm &= vm - 1ull;
        }
      };
      auto gather = [&](const int (&jj)[KC_RUNS], float (&kk)[KC_RUNS][NR], float (&ee)[KC_RUNS]) {
#pragma unroll
        for (int c = 0; c < KC_RUNS; ++c) {
          const int j = jj[c] < 0 ? 0 : jj[c];                   // an absent key re-reads slot 0's row: never used
          const float* src = nbr_tab + (uint32_t)rl_i(my_row, j) * nbr_ld;
          const uint32_t e = (uint32_t)rl_i(my_e, j);
#pragma unroll
          for (int r = 0; r < NR; ++r) kk[c][r] = src[colr[r]];
          ee[c] = Ef > 0 ? edge_feat[e * (uint32_t)Ef + (uint32_t)cole] : 0.f;
        }
      };
      auto process = [&](const int (&js)[KC_RUNS], const float (&kn)[KC_RUNS][NR], const float (&ke)[KC_RUNS]) {
        float kt[KC_RUNS][NR], ks[KC_RUNS][NR], dtv[KC_RUNS], part[KC_RUNS * H];
#pragma unroll
        for (int c = 0; c < KC_RUNS; ++c) {
          dtv[c] = rl_f(my_dt, js[c] < 0 ? 0 : js[c]);
#pragma unroll
          for (int r = 0; r < NR; ++r) {
            const float arg = pfo_time_arg(dtv[c], s_tw[lane + 64 * r], s_tb[lane + 64 * r]);
            const float u = FAST ? pfo_revolutions_fast(arg) : pfo_revolutions(arg);
            ks[c][r] = __builtin_amdgcn_sinf(u);
            kt[c][r] = __builtin_amdgcn_cosf(u);
          }
#pragma unroll
          for (int h = 0; h < H; ++h) {
            float pp = ke[c] * ge[h];
#pragma unroll
            for (int r = 0; r < NR; ++r) pp = fmaf(kn[c][r], gn[h][r], fmaf(kt[c][r], gt[h][r], pp));
            part[c * H + h] = pp;
          }
        }
        pfo_wave_sum_scalar_n<KC_RUNS * H>(part);
#pragma unroll
        for (int c = 0; c < KC_RUNS; ++c) {
          if (js[c] < 0) continue;
          const bool mine = lane == js[c] + delta;              // the lane of this key's history entry
          float cA[H], cB[H];
#pragma unroll
          for (int h = 0; h < H; ++h) {
            const float ks_h = rl_f(my_ks[h], js[c]);
            const float da = (part[c * H + h] + dsb[h]) * ks_h;
            const float aj = rl_f(my_a[h], js[c]);
            const float dscore = aj * (da - t[h]);
            cA[h] = aj * ks_h;
            cB[h] = dscore * a.scale;
            sBr[h] = mine ? sBr[h] + cB[h] : sBr[h];               // key js[c]'s share of the run's rows (flush)
#pragma unroll
            for (int r = 0; r < NR; ++r) {
              dqn[h][r] = fmaf(cB[h], kn[c][r], dqn[h][r]);
              dqt[h][r] = fmaf(cB[h], kt[c][r], dqt[h][r]);
            }
            dqe[h] = fmaf(cB[h], ke[c], dqe[h]);
          }
#pragma unroll
          for (int r = 0; r < NR; ++r) {
            float dkt = 0.f;
#pragma unroll
            for (int h = 0; h < H; ++h) dkt = fmaf(cA[h], gt[h][r], fmaf(cB[h], qt[h][r], dkt));
            const float gsin = -ks[c][r] * dkt;                 // d/d(arg) cos(arg) = -sin(arg); sin(0) = 0 on lanes beyond D
            dwc[r] = fmaf(gsin, dtv[c], dwc[r]);
            dbc[r] += gsin;
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
      };
      if (fast) walk(std::true_type{}); else walk(std::false_type{});
    }
    acc_store();                                                 // the chunk's last row sums
    flush();                                                     // the chunk's last run
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int c = lane + 64 * r;
      if (c < D) {
        if (DET) {
          a.dtime_slab[(int64_t)chunk * 2 * D + c] = (double)dwc[r];
          a.dtime_slab[(int64_t)chunk * 2 * D + D + c] = (double)dbc[r];
        } else {
          double* bin = a.dtime_part + (int64_t)(chunk & (ATTN_TIME_BINS - 1)) * 2 * D;
          atomicAdd(bin + c, (double)dwc[r]);
          atomicAdd(bin + D + c, (double)dbc[r]);
        }
      }
    }
    }   // chunks of the unit
    // deterministic mode: every slab row is written - the chunks of this unit beyond the members' count own zero rows
    if (DET)
      for (int chunk = max(n_chunks, unit * RUN_CPW); chunk < (unit + 1) * RUN_CPW; ++chunk)
        for (int c = lane; c < 2 * D; c += 64) a.dtime_slab[(int64_t)chunk * 2 * D + c] = 0.0;
  }
  // (the deterministic launch has one workgroup per POSSIBLE unit; those beyond the members' count own zero rows too)
  if (DET && (int)blockIdx.x >= n_units)
    for (int chunk = (int)blockIdx.x * RUN_CPW; chunk < ((int)blockIdx.x + 1) * RUN_CPW; ++chunk)
      for (int c = lane; c < 2 * D; c += 64) a.dtime_slab[(int64_t)chunk * 2 * D + c] = 0.0;
  if (clk_on && lane == 0) pfo_clock_end(clk, g_attn_bwd_runs_clock);
}

// (4, 4) is outside the cap: pfo_attn_bwd_runs_possible says no (the kernel would spill there)
int attn_bwd_runs_run(dim3 grid, dim3 block, size_t lds, const AttnDev& d, hipStream_t stream) {
  const bool done = attn_for_shape<ATTN_RING_MAX_NRH>(d.D, d.H, [&](auto nr, auto h) {
    if (d.det) PFO_KLAUNCH((attn_bwd_runs_kernel<nr, h, true>), grid, block, lds, stream, d);
    else PFO_KLAUNCH((attn_bwd_runs_kernel<nr, h, false>), grid, block, lds, stream, d);
  });
  PFO_REQUIRE(done, "unsupported (D, H) combination");
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}
