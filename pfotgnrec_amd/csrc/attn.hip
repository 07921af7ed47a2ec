// Neighbour-tile temporal attention (K4/K5 neighbour side).
//
// One wavefront per instance; the 64 lanes stride the feature dimension so every neighbour row is
// read as contiguous 256-byte pieces (rows of the layer-0 table are L2/Infinity-Cache resident).
// Keys are never materialised: key_j = [gathered row | edge feature | cos(fma(dt, w, b))] is formed
// in registers, used for the score, folded into the running context by an online softmax, and
// recomputed in the backward (the reference's [N,K,C] key tensor is 1.4 GB at C2).
// The K/V projections are folded: the kernel consumes qk_h = Wk_h^T Q_h and emits
// ctx_h = sum_j a_jh key_j; both projections become plain GEMMs on [N, C] operands.
//
// This file is the dispatcher and host code only: the checks, the form rules, the two launchers with their profiler brackets.
// The kernels are in attn_fwd.hip, attn_bwd.hip and attn_bwd_runs.hip; attn_dev.hpp holds what those files and this one share.
#include "attn_dev.hpp"
#include <algorithm>
#include <stdlib.h>

// shader-clock pairs (common.hpp pfo_clock_*): 0 = attention forward (ring form), 1 = run-merged backward
int pfo_attn_clock_read(double* out, int reset) {
  if (int rc = attn_fwd_clock_read(out, reset)) return rc;
  return attn_bwd_runs_clock_read(out + 2, reset);
}

// the ring form takes rows it can move 16 bytes at a time, with [node | edge] inside NR column groups and one DMA per key
static bool attn_fwd_ring_ok(const PfoAttn& a) {
  // test hook, not a tuning switch: PFO_ATTN_FWD_RING=0 sends every shape to the register form, the reference the ring form is
  // tested against (tests/test_gpu_round6.py)
  static const int on = getenv("PFO_ATTN_FWD_RING") ? atoi(getenv("PFO_ATTN_FWD_RING")) : 1;
  const int NRv = (a.D + 63) / 64;
  return on && (a.D % 4) == 0 && (a.Ef % 4) == 0 && a.D + a.Ef <= 64 * NRv && a.D + a.Ef <= 256 && (a.nbr_ld % 4) == 0 &&
         (((uintptr_t)a.nbr_tab | (uintptr_t)a.edge_feat | (uintptr_t)a.QK) & 15u) == 0 && NRv * a.H <= ATTN_RING_MAX_NRH &&
         ((a.qk_ld > 0 ? a.qk_ld : (int64_t)a.H * a.Cp) % 4) == 0;
}
static bool attn_bwd_ring_ok(const PfoAttn& a, int dmode) {
  const int NRv = (a.D + 63) / 64;
  return (dmode == 0 || dmode == 2) && (a.D % 4) == 0 && (a.Ef % 4) == 0 && a.D + a.Ef <= 64 * NRv && a.D + a.Ef <= 256 &&
         (a.nbr_ld % 4) == 0 && (((uintptr_t)a.nbr_tab | (uintptr_t)a.edge_feat) & 15u) == 0 && NRv * a.H <= ATTN_RING_MAX_NRH;
}

int pfo_attn_bwd_max_parts() { return ATTN_TIME_BINS; }
int64_t pfo_attn_bwd_det_parts(int64_t N) {
  return std::max<int64_t>(pfo_align_up(pfo_ceil_div(N, RUN_CHUNK), RUN_CPW), std::min<int64_t>(ATTN_BWD_MAX_BLOCKS, pfo_ceil_div(N, 4)));
}

static void to_dev(const PfoAttn& a, AttnDev& d) {
  d.N = a.N; d.K = a.K; d.D = a.D; d.Ef = a.Ef; d.H = a.H; d.Cp = a.Cp;
  d.QK = a.QK; d.qk_row = a.qk_row; d.qk_ld = a.qk_ld > 0 ? a.qk_ld : (int64_t)a.H * a.Cp; d.nbr_tab = a.nbr_tab; d.nbr_ld = a.nbr_ld; d.nbr_row = a.nbr_row; d.nbr_row_base = a.nbr_row_base; d.nbr_relu = a.nbr_relu;
  d.nbr_ids = a.nbr_ids; d.edge_feat = a.edge_feat; d.eidx = a.eidx; d.dt = a.dt; d.tw = a.tw; d.tb = a.tb;
  d.scale = a.scale; d.dropout_p = a.dropout_p; d.seed = a.seed; d.offset = a.offset; d.offset_dev = a.offset_dev; d.keep_inject = a.keep_inject;
  d.xcd_g = 0;
  d.ctx = a.ctx; d.attw = a.attw; d.inv = a.inv;
  d.dctx = a.dctx; d.dQK = a.dQK; d.d_nbr = a.d_nbr; d.d_nbr_ld = a.d_nbr_ld; d.d_nbr_rep = a.d_nbr_rep; d.d_nbr_nrep = a.d_nbr_nrep > 0 ? a.d_nbr_nrep : 1;
  d.dtime_part = a.dtime_part;
  d.det = a.det; d.dtime_slab = a.dtime_slab; d.dqk_live = a.dqk_live;
  d.members = a.members; d.seg_ptr = a.seg_ptr; d.n_rows = a.n_rows; d.run_cnt = a.run_cnt;
}

static int check_common(const PfoAttn& a) {
  PFO_REQUIRE(a.N > 0 && a.K >= 1 && a.K <= PFO_MAX_NEIGHBORS, "bad N / K");
  PFO_REQUIRE(a.D >= 1 && a.D <= 256, "D must be <= 256");
  PFO_REQUIRE(a.Ef >= 0 && a.Ef <= 64, "Ef must be <= 64");
  PFO_REQUIRE(a.H == 1 || a.H == 2 || a.H == 4, "n_heads must be 1, 2 or 4");
  PFO_REQUIRE(a.QK && a.nbr_tab && a.nbr_ids && a.eidx && a.dt && a.tw && a.tb && a.ctx && a.attw && a.inv, "null input");
  PFO_REQUIRE(a.Ef == 0 || a.edge_feat, "null edge features");
  PFO_REQUIRE(a.dropout_p >= 0.f && a.dropout_p < 1.f, "dropout must be in [0, 1)");
  PFO_REQUIRE(a.Cp >= 2 * a.D + a.Ef + 2 && (a.Cp % 4) == 0, "Cp must hold C + 2 columns and be a multiple of 4");
  // the kernels address the gathered rows with 32-bit element offsets
  PFO_REQUIRE(a.nbr_rows > 0 && (uint64_t)a.nbr_rows * (uint64_t)a.nbr_ld < (1ull << 32), "neighbour table too large for 32-bit row offsets");
  PFO_REQUIRE(a.Ef == 0 || (a.edge_rows > 0 && (uint64_t)a.edge_rows * (uint64_t)a.Ef < (1ull << 32)), "edge feature table too large for 32-bit row offsets");
  return PFO_OK;
}

static int attn_fwd_form(const PfoAttn& a) { return attn_fwd_ring_ok(a) ? PFO_ATTN_FORM_FWD_RING : PFO_ATTN_FORM_FWD_REG; }
int pfo_attn_fwd_launch(const PfoAttn& a, hipStream_t stream) {
  if (int rc = check_common(a)) return rc;
  AttnDev d;
  to_dev(a, d);
  // algorithmic bytes per instance: K gathered rows + edge feature + (eidx, dt, id), qk in, ctx + weights out
  const double C = 2.0 * a.D + a.Ef;
  const double bytes = (double)a.N * (a.K * (4.0 * a.D + 4.0 * a.Ef + 12.0) + 2.0 * a.H * C * 4.0 + 4.0 * a.H * a.K);
  pfo_prof_begin(stream);
  if (int rc = attn_fwd_run(attn_fwd_form(a), dim3((unsigned)pfo_ceil_div(a.N, 4)), dim3(256), d, stream)) return rc;
  pfo_prof_end(PFO_PROF_ATTN_FWD, bytes, stream);
  return PFO_OK;
}

// the step's dropout multipliers, written out (include/pfotgn.h pfo_attn_dropout_mask; the kernel is in attn_fwd.hip)
extern "C" int pfo_attn_dropout_mask(uint64_t seed, uint64_t offset, int64_t N, int32_t K, int32_t H, float p, float* out,
                                     void* stream) {
  PFO_REQUIRE(out != nullptr && N >= 0, "bad arguments");
  PFO_REQUIRE(K >= 1 && K <= 64, "K must be in [1, 64] (one keep word per lane of a wavefront)");
  PFO_REQUIRE(H == 1 || H == 2 || H == 4, "n_heads must be 1, 2 or 4");
  PFO_REQUIRE(p >= 0.f && p < 1.f, "dropout must be in [0, 1)");
  if (N == 0) return PFO_OK;
  const int64_t total = N * K;
  const unsigned grid = (unsigned)std::min<int64_t>(4096, pfo_ceil_div(total, 256));
  return attn_dropout_mask_run(dim3(grid), dim3(256), seed, offset, N, (int)K, (int)H, p, out, (hipStream_t)stream);
}

bool pfo_attn_bwd_runs_possible(int K, int D, int H) {
  // D > 192 with four heads (NR = 4, H = 4) needs more than the 256 registers a lane can have: the run-merged kernel would spill
  // 160-176 B per lane to scratch there - that shape takes the per-instance kernel (no spill), like uniform sampling does
  const bool fits = !(D > 192 && H == 4);
  return K <= 64 && fits;
}
bool pfo_attn_bwd_uses_runs(const PfoAttn& a) {
  // (the staging LDS-DMA moves 16 bytes per lane: rows must start on 16-byte boundaries)
  const int64_t qk_ld = a.qk_ld > 0 ? a.qk_ld : (int64_t)a.H * a.Cp;
  const bool aligned = (qk_ld % 4) == 0 && (((uintptr_t)a.QK | (uintptr_t)a.dctx | (uintptr_t)a.ctx) & 15u) == 0;
  return a.d_nbr && a.nbr_row && pfo_attn_bwd_runs_possible(a.K, a.D, a.H) && a.members && a.seg_ptr && a.n_rows && a.qk_row && a.run_cnt &&
         a.dqk_live && aligned;
}

// what happens to the neighbour-row gradients (DMODE of the kernels): 0 none, 1 added into the rows nbr_row names, 2 plain stores
static int attn_bwd_dmode(const PfoAttn& a) { return !a.d_nbr ? 0 : (a.nbr_row ? 1 : 2); }
static int attn_bwd_form(const PfoAttn& a) {
  const int dmode = attn_bwd_dmode(a);
  if (pfo_attn_bwd_uses_runs(a)) return PFO_ATTN_FORM_BWD_RUNS;
  if (attn_bwd_ring_ok(a, dmode)) return dmode == 0 ? PFO_ATTN_FORM_BWD_RING_NONE : PFO_ATTN_FORM_BWD_RING_DIRECT;
  if (dmode == 0) return PFO_ATTN_FORM_BWD_NONE;
  if (dmode == 1) return a.det ? PFO_ATTN_FORM_BWD_DET : PFO_ATTN_FORM_BWD_ATOMIC;
  return PFO_ATTN_FORM_BWD_DIRECT;
}
int pfo_attn_form(const PfoAttn& a, bool backward) {
  if (check_common(a)) return -1;
  return backward ? attn_bwd_form(a) : attn_fwd_form(a);
}

int pfo_attn_bwd_launch(const PfoAttn& a, int* n_parts, hipStream_t stream) {
  if (int rc = check_common(a)) return rc;
  PFO_REQUIRE(a.dctx && a.dQK && a.dtime_part, "null backward buffers");
  PFO_REQUIRE(!a.det || a.dtime_slab, "deterministic mode needs the slab");
  const int form = attn_bwd_form(a);
  AttnDev d;
  to_dev(a, d);
  const int grid = (int)std::min<int64_t>(ATTN_BWD_MAX_BLOCKS, pfo_ceil_div(a.N, 4));   // (deterministic: the slab's row count is fixed)
  // rows read again + their gradient rows written/added, qk + dctx + ctx in, dqk out
  const double C = 2.0 * a.D + a.Ef;
  const double bytes = (double)a.N * (a.K * (8.0 * a.D + 4.0 * a.Ef + 12.0) + 4.0 * a.H * C * 4.0 + 4.0 * a.H * a.K);
  // the run-merged kernel's staging image: three rows of H Cp floats + (4 + H) metadata arrays of K words (attn_bwd_runs_kernel)
  const size_t run_lds = 3 * (size_t)a.H * a.Cp * 4 + (size_t)(4 + a.H) * a.K * 4 + (size_t)pfo_align_up(4 * a.K, 16);   // (+ K injected keep bytes, one dword each)
  if (form == PFO_ATTN_FORM_BWD_RUNS) {
    // run-merged form: single-wavefront workgroups, one unit of chunks each (the grid covers every possible unit, so the
    // kernel's grid-stride loop runs once)
    // (16 chunks per XCD turn: FETCH 625 -> 487 MB per launch, 512 at 4; the launch time does not move)
    d.xcd_g = a.det ? 0 : 16;                                  // (deterministic mode: slab row = chunk = workgroup id)
    int64_t all_units = pfo_ceil_div(pfo_ceil_div(a.N, RUN_CHUNK), RUN_CPW);       // a wavefront takes RUN_CPW chunks
    if (d.xcd_g > 0) all_units = pfo_align_up(all_units, 8 * d.xcd_g);
    const int rgrid = (int)all_units;
    pfo_prof_begin(stream);
    if (int rc = attn_bwd_runs_run(dim3((unsigned)rgrid), dim3(64), run_lds, d, stream)) return rc;
    pfo_prof_end(PFO_PROF_ATTN_BWD_RUNS, bytes, stream);
    if (n_parts) *n_parts = a.det ? rgrid * RUN_CPW : ATTN_TIME_BINS;   // deterministic: slab rows written (one per chunk, RUN_CPW per workgroup)
    return PFO_OK;
  }
  pfo_prof_begin(stream);
  if (int rc = attn_bwd_run(form, dim3((unsigned)grid), dim3(256), d, stream)) return rc;
  pfo_prof_end(PFO_PROF_ATTN_BWD, bytes, stream);
  if (n_parts) *n_parts = a.det ? grid : ATTN_TIME_BINS;
  return PFO_OK;
}
