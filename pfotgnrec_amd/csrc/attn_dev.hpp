// What the attention's translation units share (internal): attn.hip, the dispatcher, is host code and holds no kernel; each
// kernel family has a file of its own (attn_fwd.hip, attn_bwd.hip, attn_bwd_runs.hip).  Device helpers are header-only and
// __forceinline__: no relocatable device code.  A kernel template is launched from the file that defines it, through the
// launch functions declared at the end.
#pragma once
#include "attn.hpp"
#include "attn_shape.hpp"
#include <string.h>

struct AttnDev {
  int N, K, D, Ef, H, Cp;
  const float* QK; const int32_t* qk_row; int64_t qk_ld; const float* nbr_tab; int64_t nbr_ld; const int32_t* nbr_row; int64_t nbr_row_base; int nbr_relu;
  const int32_t* nbr_ids; const float* edge_feat; const int32_t* eidx; const float* dt; const float* tw; const float* tb;
  float scale, dropout_p; uint64_t seed, offset; const uint64_t* offset_dev; const uint8_t* keep_inject;
  float* ctx; float* attw; uint8_t* inv;
  const float* dctx; float* dQK; float* d_nbr; int64_t d_nbr_ld; double* dtime_part;
  int64_t d_nbr_rep;  // DMODE 1: floats between the per-XCD replicas of the gradient table (0: one table)
  int d_nbr_nrep;     // ... and how many of them are in use (a power of two)
  // run-merged layer-1 backward: instances in (table row, run key) order, seg_ptr[*n_rows] of them
  const int32_t* members; const int32_t* seg_ptr; const int32_t* n_rows; const int32_t* run_cnt;
  int det; double* dtime_slab;   // deterministic mode (attn.hpp)
  uint8_t* dqk_live;             // run-merged kernel: [members] 1 = dQK row m holds a sum, 0 = folded into a later row / nothing
  int xcd_g;    // run-merged backward: G consecutive chunks of members per XCD turn (0 = chunks round-robin over the XCDs)
};

// deterministic mode: a gradient element is added as 2^-40 fixed point - integer addition does not depend on the order
__device__ __forceinline__ void det_add(float* table, int64_t idx, float v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(table) + idx, (unsigned long long)__double2ll_rn((double)v * PFO_DET_SCALE));
}

// dropout keep-bits for slot `lane` of instance n: bit h = keep for head h (H <= 4)
__device__ __forceinline__ unsigned attn_keep_bits(uint64_t seed, uint64_t offset, int64_t n, int lane, float p) {
  if (p <= 0.f) return 0xFu;
  const pfo_u4 r = pfo_philox(seed, (uint64_t)n * 64ull + (uint64_t)lane, offset);
  const uint32_t thr = (uint32_t)fminf(p * 4294967296.0f, 4294967040.0f);
  return (r.x >= thr ? 1u : 0u) | (r.y >= thr ? 2u : 0u) | (r.z >= thr ? 4u : 0u) | (r.w >= thr ? 8u : 0u);
}

// ... or the caller's injected decisions (parity tests): one wave-uniform test per instance
__device__ __forceinline__ unsigned attn_keep_for(const AttnDev& a, uint64_t rng_off, int64_t n, int lane) {
  if (a.keep_inject && a.dropout_p > 0.f) return lane < a.K ? (unsigned)a.keep_inject[n * a.K + lane] : 0xFu;
  return attn_keep_bits(a.seed, rng_off, n, lane, a.dropout_p);
}

// Keys are processed in chunks of KC: all gathers of a chunk are issued back to back (one memory latency per
// chunk instead of one per key), the chunk's KC*H dot-product butterflies are interleaved (6 dependent shuffle
// stages per chunk instead of per key), then the online-softmax state is advanced key by key.  Per-slot metadata
// (row, edge id, dt, validity) is loaded once, one slot per lane, and broadcast with v_readlane.
constexpr int KC_FWD = 2;
constexpr int KC_BWD = 2;

__device__ __forceinline__ int rl_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float rl_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// s_waitcnt vmcnt(N) for a compile-time N: the key rings count their LDS-DMA loads exactly (attn_fwd.hip, attn_bwd.hip)
template <int N> __device__ __forceinline__ void pfo_wait_vm() {
  static_assert(N >= 0 && N <= 14 && N % 2 == 0, "vmcnt");
  if constexpr (N == 14) asm volatile("s_waitcnt vmcnt(14)" ::: "memory");
  else if constexpr (N == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
  else if constexpr (N == 10) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
  else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
// wait until at most 2 * pairs_behind DMAs are outstanding (pairs_behind <= P = the ring's pairs - 1, wave-uniform)
template <int P>
__device__ __forceinline__ void pfo_wait_pairs(int pairs_behind) {
  if constexpr (P <= 0) { pfo_wait_vm<0>(); }
  else {
    if (pairs_behind >= P) pfo_wait_vm<2 * P>();
    else pfo_wait_pairs<P - 1>(pairs_behind);
  }
}

constexpr int ATTN_BWD_MAX_BLOCKS = 4096;
constexpr int RUN_CHUNK = 4;    // measured at C2 (round 2): 2: 399, 3: 370, 4: 365, 6: 402, 8: 417 us (a wavefront walks its chunk serially:
                                // long chunks merge more atomics but leave a tail)
constexpr int RUN_CPW = 1;      // consecutive chunks per wavefront: one prologue (member ids -> query rows / counts) for all their members

// One shader-clock pair (common.hpp pfo_clock_*).  A device symbol and its reader share a translation unit, so every kernel
// file that stamps a pair keeps the symbol and hands it to this reader; attn.hip's pfo_attn_clock_read joins them.
static inline int attn_clock_pair_read(const void* symbol, double* out /* [2] */, int reset) {
  unsigned long long h[2];
  if (hipMemcpyFromSymbol(h, symbol, sizeof(h)) != hipSuccess) return PFO_ERR_HIP;
  out[0] = (double)h[0]; out[1] = (double)h[1];
  if (reset) { memset(h, 0, sizeof(h)); if (hipMemcpyToSymbol(symbol, h, sizeof(h)) != hipSuccess) return PFO_ERR_HIP; }
  return PFO_OK;
}
int attn_fwd_clock_read(double* out, int reset);        // attn_fwd.hip: pair 0, the forward's ring form
int attn_bwd_runs_clock_read(double* out, int reset);   // attn_bwd_runs.hip: pair 1, the run-merged backward

// The launch functions, one per dispatch site of attn.hip: each takes the finished form (a PFO_ATTN_FORM_* the file's kernels
// answer to), the launch geometry and the filled argument block, and does PFO_KLAUNCH + PFO_LAUNCH_CHECK for the (NR, H)
// instance attn_for_shape picks - no argument checks, no form decisions, no profiler calls (those bracket the call in attn.hip).
int attn_fwd_run(int form, dim3 grid, dim3 block, const AttnDev& d, hipStream_t stream);                        // attn_fwd.hip
int attn_dropout_mask_run(dim3 grid, dim3 block, uint64_t seed, uint64_t offset, int64_t N, int K, int H, float p, float* out,
                          hipStream_t stream);                                                                  // attn_fwd.hip
int attn_bwd_run(int form, dim3 grid, dim3 block, const AttnDev& d, hipStream_t stream);                        // attn_bwd.hip
int attn_bwd_runs_run(dim3 grid, dim3 block, size_t lds, const AttnDev& d, hipStream_t stream);                 // attn_bwd_runs.hip
