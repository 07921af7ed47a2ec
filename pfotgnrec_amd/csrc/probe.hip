// Debug / test probes of the internal contraction interface (gemm.hpp), of the attention interface (attn.hpp) and of the
// memory-side interface (memory.hpp: the grouping the run-merged attention backward consumes, and one probe per launcher of
// the compaction, state-update and small-op kernels): the flat C structs of include/pfotgn.h copied field
// for field into the internal ones and handed to the internal launchers unchanged.  No logic of their own beyond null and
// count checks - what a probe computes is what tgn.hip gets from the same launcher.
#include "gemm.hpp"
#include "attn.hpp"
#include "memory.hpp"

static void to_gemm(const pfo_gemm_desc& s, PfoGemm& g) {
  for (int i = 0; i < 2; ++i) {
    g.A[i] = s.A[i]; g.lda[i] = s.lda[i]; g.a_idx[i] = s.a_idx[i];
    g.B[i] = s.B[i]; g.ldb[i] = s.ldb[i]; g.K[i] = s.K[i];
    g.a_bs[i] = s.a_bs[i]; g.b_bs[i] = s.b_bs[i];
  }
  g.b_idx = s.b_idx;
  g.C = s.C; g.ldc = s.ldc;
  g.bias = s.bias; g.row_scale = s.row_scale; g.rs_ld = s.rs_ld; g.row_zero = s.row_zero;
  g.relu_src = s.relu_src; g.relu_ld = s.relu_ld;
  g.add_src = s.add_src; g.add_ld = s.add_ld; g.add_idx = s.add_idx;
  g.M = s.M; g.N = s.N; g.m_dev = s.m_dev;
  g.relu = s.relu; g.accumulate = s.accumulate; g.a_kmajor = s.a_kmajor; g.b_kmajor = s.b_kmajor;
  g.batch = s.batch; g.c_bs = s.c_bs; g.bias_bs = s.bias_bs; g.rs_bs = s.rs_bs;
  g.slabs = s.slabs; g.slab_floats = s.slab_floats;
  g.b_img = s.b_img; g.b_img2 = s.b_img2; g.bx_force = s.bx_force;
}

extern "C" int pfo_debug_gemm(const pfo_gemm_desc* g, void* stream) {
  PFO_REQUIRE(g, "null descriptor");
  PfoGemm q;
  to_gemm(*g, q);
  return pfo_gemm_launch(q, (hipStream_t)stream);
}

#define PROBE_MULTI_MAX 32
extern "C" int pfo_debug_gemm_multi(const pfo_gemm_desc* list, int32_t n, void* stream) {
  PFO_REQUIRE(list && n >= 1 && n <= PROBE_MULTI_MAX, "bad problem list");
  PfoGemm q[PROBE_MULTI_MAX];
  for (int i = 0; i < n; ++i) to_gemm(list[i], q[i]);
  return pfo_gemm_multi_launch(q, n, (hipStream_t)stream);
}

#define PROBE_TN_MAX 16
static void to_tn(const pfo_tn_desc* probs, int n, PfoTnProblem* q) {
  for (int i = 0; i < n; ++i) {
    const pfo_tn_desc& s = probs[i];
    q[i].A = s.A; q[i].lda = s.lda; q[i].B = s.B; q[i].ldb = s.ldb; q[i].b_idx = s.b_idx; q[i].M = s.M; q[i].N = s.N;
    q[i].C = s.C; q[i].ldc = s.ldc; q[i].c_accumulate = s.c_accumulate;
    q[i].bias_out = s.bias_out; q[i].bias_accumulate = s.bias_accumulate;
  }
}
extern "C" int pfo_debug_gemm_tn_group(const pfo_tn_desc* probs, int32_t n, int32_t K, const int32_t* k_dev, float* slabs,
                                       int64_t slab_floats, void* stream) {
  PFO_REQUIRE(probs && n >= 1 && n <= PROBE_TN_MAX, "bad problem list");
  PfoTnProblem q[PROBE_TN_MAX];
  to_tn(probs, n, q);
  return pfo_gemm_tn_group_launch(q, n, K, k_dev, slabs, slab_floats, (hipStream_t)stream);
}

extern "C" int32_t pfo_debug_gemm_plan(const pfo_gemm_desc* g, int32_t* out) {
  if (!g || !out) { pfo_set_error("%s: null argument", __func__); return -1; }
  PfoGemm q;
  to_gemm(*g, q);
  return pfo_gemm_plan(q, out);
}
extern "C" int32_t pfo_debug_gemm_tn_group_plan(const pfo_tn_desc* probs, int32_t n, int32_t K, int64_t slab_floats, int32_t* out) {
  if (!probs || n < 1 || n > PROBE_TN_MAX || !out) { pfo_set_error("%s: bad problem list", __func__); return -1; }
  PfoTnProblem q[PROBE_TN_MAX];
  to_tn(probs, n, q);
  return pfo_gemm_tn_group_plan(q, n, K, slab_floats, out);
}

extern "C" int64_t pfo_debug_bimg_bytes(int32_t N, int32_t K) {
  if (N <= 0 || K <= 0) { pfo_set_error("%s: bad sizes", __func__); return -1; }
  return pfo_bimg_bytes(N, K);
}
extern "C" int64_t pfo_debug_gru_img_bytes(int32_t D, int32_t K) {
  if (D <= 0 || K <= 0) { pfo_set_error("%s: bad sizes", __func__); return -1; }
  return pfo_gru_img_bytes(D, K);
}

extern "C" int pfo_debug_bimg(const pfo_bimg_desc* list, int32_t n, void* stream) {
  PFO_REQUIRE(list && n >= 1 && n <= PFO_BIMG_MAX, "bad image list");
  PfoBimg q[PFO_BIMG_MAX];
  for (int i = 0; i < n; ++i) {
    const pfo_bimg_desc& s = list[i];
    q[i].src = s.src; q[i].ld = s.ld; q[i].N = s.N; q[i].K = s.K; q[i].trans = s.trans; q[i].dst = s.dst;
    q[i].row0 = s.row0; q[i].rows_total = s.rows_total; q[i].last = s.last; q[i].gate = s.gate; q[i].gate_D = s.gate_D;
  }
  return pfo_bimg_launch(q, n, (hipStream_t)stream);
}

extern "C" int pfo_debug_msg_mlp_fwd(const pfo_msg_mlp_desc* f, void* stream) {
  PFO_REQUIRE(f, "null descriptor");
  PfoMsgMlp q;
  q.raw = f->raw; q.ld_raw = f->ld_raw; q.touched = f->touched; q.hm = f->hm; q.img_w1 = f->img_w1; q.img_w2 = f->img_w2;
  q.b1 = f->b1; q.b2 = f->b2; q.hid = f->hid; q.msg_out = f->msg_out; q.Mr = f->Mr; q.Hm = f->Hm; q.Md = f->Md;
  q.cap_rows = f->cap_rows; q.n_rows = f->n_rows;
  return pfo_msg_mlp_fwd_launch(q, (hipStream_t)stream);
}

extern "C" int pfo_debug_msg_mlp_bwd(const pfo_msg_mlp_bwd_desc* f, void* stream) {
  PFO_REQUIRE(f, "null descriptor");
  PfoMsgMlpBwd q;
  q.dgi = f->dgi; q.hid = f->hid; q.img_wihT = f->img_wihT; q.img_w2T = f->img_w2T; q.d_m = f->d_m; q.d_hid = f->d_hid;
  q.D3 = f->D3; q.Hm = f->Hm; q.Md = f->Md; q.cap_rows = f->cap_rows; q.n_rows = f->n_rows;
  return pfo_msg_mlp_bwd_launch(q, (hipStream_t)stream);
}

extern "C" int pfo_debug_gru_fused(const pfo_gru_desc* f, void* stream) {
  PFO_REQUIRE(f, "null descriptor");
  PfoGruFused q;
  q.msg_rows = f->msg_rows; q.K_msg = f->K_msg; q.h_rows = f->h_rows; q.img_ih = f->img_ih; q.img_hh = f->img_hh;
  q.b_ih = f->b_ih; q.b_hh = f->b_hh; q.hm = f->hm; q.touched = f->touched; q.node_feat = f->node_feat;
  q.upd_mem = f->upd_mem; q.h0_tab = f->h0_tab; q.gates = f->gates; q.D = f->D; q.cap_rows = f->cap_rows; q.n_rows = f->n_rows;
  q.gather = f->gather;
  return pfo_gru_fused_launch(q, (hipStream_t)stream);
}

extern "C" int pfo_debug_rank1_multi(const pfo_rank1_desc* list, int32_t n, void* stream) {
  PFO_REQUIRE(list && n >= 1 && n <= PFO_RANK1_MAX, "bad rank-1 list");
  PfoRank1 q[PFO_RANK1_MAX];
  for (int i = 0; i < n; ++i) {
    const pfo_rank1_desc& s = list[i];
    q[i].u = s.u; q[i].ldu = s.ldu; q[i].v = s.v; q[i].ldv = s.ldv; q[i].M = s.M; q[i].N = s.N; q[i].out = s.out; q[i].ldo = s.ldo;
    q[i].reps = s.reps; q[i].u_rs = s.u_rs; q[i].v_rs = s.v_rs;
  }
  return pfo_rank1_multi_launch(q, n, (hipStream_t)stream);
}

extern "C" int pfo_debug_sum_slabs(const pfo_sum_slabs_desc* list, int32_t n, void* stream) {
  PFO_REQUIRE(list && n >= 1 && n <= PFO_SUM_SLABS_MAX, "bad slab list");
  PfoSumSlabs q[PFO_SUM_SLABS_MAX];
  for (int i = 0; i < n; ++i) {
    q[i].dst = list[i].dst; q[i].src = list[i].src; q[i].stride = list[i].stride; q[i].count = list[i].count;
    q[i].n_slabs = list[i].n_slabs; q[i].accumulate = list[i].accumulate;
  }
  return pfo_sum_slabs_launch(q, n, (hipStream_t)stream);
}

// ---- the internal attention interface (attn.hpp) and the grouping its run-merged backward consumes (memory.hpp)
static void to_attn(const pfo_attn_desc& s, PfoAttn& a) {
  a.N = s.N; a.K = s.K; a.D = s.D; a.Ef = s.Ef; a.H = s.H; a.Cp = s.Cp;
  a.QK = s.QK; a.qk_row = s.qk_row; a.qk_ld = s.qk_ld;
  a.nbr_tab = s.nbr_tab; a.nbr_ld = s.nbr_ld; a.nbr_row = s.nbr_row; a.nbr_row_base = s.nbr_row_base;
  a.nbr_rows = s.nbr_rows; a.edge_rows = s.edge_rows; a.nbr_relu = s.nbr_relu;
  a.nbr_ids = s.nbr_ids; a.edge_feat = s.edge_feat; a.eidx = s.eidx; a.dt = s.dt; a.tw = s.tw; a.tb = s.tb;
  a.scale = s.scale; a.dropout_p = s.dropout_p; a.seed = s.seed; a.offset = s.offset; a.offset_dev = s.offset_dev;
  a.keep_inject = s.keep_inject;
  a.ctx = s.ctx; a.attw = s.attw; a.inv = s.inv;
  a.dctx = s.dctx; a.dQK = s.dQK; a.d_nbr = s.d_nbr; a.d_nbr_ld = s.d_nbr_ld; a.d_nbr_rep = s.d_nbr_rep; a.d_nbr_nrep = s.d_nbr_nrep;
  a.dtime_part = s.dtime_part; a.det = s.det; a.dtime_slab = s.dtime_slab; a.dqk_live = s.dqk_live;
  a.members = s.members; a.seg_ptr = s.seg_ptr; a.n_rows = s.n_rows; a.run_cnt = s.run_cnt;
}

extern "C" int pfo_debug_attn_fwd(const pfo_attn_desc* desc, void* stream) {
  PFO_REQUIRE(desc, "null descriptor");
  PfoAttn a;
  to_attn(*desc, a);
  return pfo_attn_fwd_launch(a, (hipStream_t)stream);
}
extern "C" int pfo_debug_attn_bwd(const pfo_attn_desc* desc, int32_t* n_parts, void* stream) {
  PFO_REQUIRE(desc, "null descriptor");
  PfoAttn a;
  to_attn(*desc, a);
  int parts = 0;
  const int rc = pfo_attn_bwd_launch(a, &parts, (hipStream_t)stream);
  if (n_parts) *n_parts = parts;
  return rc;
}
extern "C" int64_t pfo_debug_attn_det_parts(int64_t N) {
  if (N <= 0) { pfo_set_error("%s: bad size", __func__); return -1; }
  return pfo_attn_bwd_det_parts(N);
}
extern "C" int32_t pfo_debug_attn_form(const pfo_attn_desc* desc, int32_t backward) {
  if (!desc) { pfo_set_error("%s: null descriptor", __func__); return -1; }
  PfoAttn a;
  to_attn(*desc, a);
  return pfo_attn_form(a, backward != 0);
}

extern "C" int64_t pfo_debug_seg_scratch_ints(int32_t cap_rows) {
  if (cap_rows <= 0) { pfo_set_error("%s: bad size", __func__); return -1; }
  return pfo_seg_scratch_ints(cap_rows);
}
extern "C" int64_t pfo_debug_seg_of_ints(int64_t n_members) {
  if (n_members <= 0) { pfo_set_error("%s: bad size", __func__); return -1; }
  return pfo_seg_of_ints(n_members);
}
extern "C" int pfo_debug_seg_build(const int32_t* idx, const int32_t* nodes, int32_t N, int32_t cap_rows, const int32_t* key_src,
                                   int32_t* seg_ptr, int32_t* members, int32_t* seg_of, int32_t* scratch, int64_t scratch_ints,
                                   void* stream) {
  PFO_REQUIRE(N > 0 && cap_rows > 0 && scratch, "bad arguments");
  const int64_t scan = pfo_seg_scratch_ints(cap_rows);
  PFO_REQUIRE(scratch_ints >= scan + 2 * ((int64_t)cap_rows + 1) + N, "short scratch");
  int32_t* cursor = scratch + scan;
  int32_t* tmp = cursor + 2 * ((int64_t)cap_rows + 1);
  return pfo_seg_build_launch(idx, nodes, N, cap_rows, key_src, seg_ptr, cursor, tmp, members, seg_of, scratch, (hipStream_t)stream);
}

// ---- the memory-side interface (memory.hpp): one probe per launcher, the arguments handed on unchanged.  The path queries
// answer from the functions the launchers (or the kernels' loop bounds) are written with.
extern "C" int64_t pfo_debug_compact_scratch_ints(int32_t n_nodes) {
  if (n_nodes <= 0) { pfo_set_error("%s: bad size", __func__); return -1; }
  return pfo_compact_scratch_ints(n_nodes);
}
extern "C" int pfo_debug_touch_compact(const int32_t* nodes0, int64_t n0, const int32_t* extra, int64_t n_extra, int32_t n_nodes,
                                       int32_t* mark, int32_t* slot, int32_t* touched_ids, int32_t* n_counts, int32_t* scratch,
                                       int64_t scratch_ints, int32_t marks_are_zero, int32_t marked, void* stream) {
  PFO_REQUIRE(n_nodes > 0 && n0 >= 0 && n_extra >= 0 && (n_extra == 0 || extra), "bad arguments");
  PFO_REQUIRE(scratch && scratch_ints >= pfo_compact_scratch_ints(n_nodes), "short scratch");
  return pfo_touch_compact_launch(nodes0, n0, extra, n_extra, n_nodes, mark, slot, touched_ids, n_counts, scratch,
                                  marks_are_zero != 0, marked != 0, (hipStream_t)stream);
}
extern "C" int pfo_debug_pack_remap(const float* msg_table, int32_t M, const float* memory, int32_t D, const uint8_t* has_msg,
                                    const int32_t* touched_ids, const int32_t* n_touched, int32_t cap, float* msg_rows,
                                    float* h_rows, uint8_t* hm, const int32_t* nodes0, int64_t n0, const int32_t* slot,
                                    int32_t* idx0, void* stream) {
  PFO_REQUIRE(cap > 0 && D > 0 && M >= 0, "bad sizes");
  return pfo_pack_remap_launch(msg_table, M, memory, D, has_msg, touched_ids, n_touched, cap, msg_rows, h_rows, hm, nodes0, n0,
                               slot, idx0, (hipStream_t)stream);
}
extern "C" int32_t pfo_debug_gru_gates_bwd_vec(const float* gates, const float* dgi, const float* dgh, const float* h_rows,
                                               int32_t D, const float* d_h0, int64_t rep_stride, const float* d_extra) {
  return pfo_gru_gates_bwd_vec(gates, dgi, dgh, h_rows, D, d_h0, rep_stride, d_extra) ? 1 : 0;
}
extern "C" int pfo_debug_gru_gates_bwd(const float* gates, float* dgi, float* dgh, const float* h_rows, const uint8_t* hm,
                                       const int32_t* n_touched, int32_t cap, int32_t D, const float* d_h0, int32_t n_rep,
                                       int64_t rep_stride, const float* d_extra, int32_t det, void* stream) {
  PFO_REQUIRE(gates && dgi && dgh && h_rows && hm && n_touched && d_h0, "null argument");
  PFO_REQUIRE(cap > 0 && D > 0 && n_rep >= 1 && rep_stride >= 0, "bad sizes");
  return pfo_gru_gates_bwd_launch(gates, dgi, dgh, h_rows, hm, n_touched, cap, D, d_h0, n_rep, rep_stride, d_extra, det,
                                  (hipStream_t)stream);
}
extern "C" int pfo_debug_zero_rows(float* dst, const int32_t* n_rows, int32_t cap_rows, int32_t D, int32_t n_rep, int64_t rep_stride,
                                   void* stream) {
  PFO_REQUIRE(dst && n_rows, "null argument");
  PFO_REQUIRE(cap_rows > 0 && D > 0 && n_rep >= 1 && rep_stride >= 0, "bad sizes");
  return pfo_zero_rows_launch(dst, n_rows, cap_rows, D, n_rep, rep_stride, (hipStream_t)stream);
}
extern "C" int pfo_debug_persist(const int32_t* src, const int32_t* dst, int32_t B, const int32_t* slot, const float* upd_mem,
                                 const uint8_t* has_msg, const float* msg_time, float* memory, float* last_update, int32_t D,
                                 int32_t* winner, void* stream) {
  PFO_REQUIRE(src && dst && slot && upd_mem && has_msg && msg_time && memory && last_update, "null argument");
  PFO_REQUIRE(B > 0 && D > 0, "bad sizes");
  return pfo_persist_launch(src, dst, B, slot, upd_mem, has_msg, msg_time, memory, last_update, D, winner, (hipStream_t)stream);
}
extern "C" int32_t pfo_debug_msg_store_needs_winner(int32_t B) {
  if (B <= 0) { pfo_set_error("%s: bad size", __func__); return -1; }
  return pfo_msg_store_needs_winner(B) ? 1 : 0;
}
extern "C" int pfo_debug_msg_store(const int32_t* src, const int32_t* dst, const double* ts, const int32_t* eidx, int32_t B,
                                   const float* memory, const float* last_update, const float* edge_feat, const float* tw,
                                   const float* tb, int32_t D, int32_t Ef, float* msg_table, float* msg_time, uint8_t* has_msg,
                                   int32_t* winner, void* stream) {
  PFO_REQUIRE(src && dst && ts && eidx && memory && last_update && tw && tb && msg_table && msg_time && has_msg, "null argument");
  PFO_REQUIRE(B > 0 && D > 0 && Ef >= 0 && (Ef == 0 || edge_feat), "bad sizes");
  return pfo_msg_store_launch(src, dst, ts, eidx, B, memory, last_update, edge_feat, tw, tb, D, Ef, msg_table, msg_time, has_msg,
                              winner, (hipStream_t)stream);
}
extern "C" int pfo_debug_observe_select(const int32_t* src, const int32_t* dst, int32_t B, const uint8_t* has_msg, int32_t* rep,
                                        int32_t base, int32_t* slot, int32_t* touched, int32_t* n_out, void* stream) {
  return pfo_observe_select_launch(src, dst, B, has_msg, rep, base, slot, touched, n_out, (hipStream_t)stream);
}
extern "C" int32_t pfo_debug_scan_sweeps(int64_t n) {
  if (n <= 0 || n >= ((int64_t)1 << 31)) { pfo_set_error("%s: bad size", __func__); return -1; }
  return pfo_scan_sweeps(n);
}
extern "C" int pfo_debug_iscan(const int32_t* in, int64_t n, int32_t* out, int32_t* scratch, int64_t scratch_ints, void* stream) {
  PFO_REQUIRE(n > 0, "bad size");
  PFO_REQUIRE(scratch && scratch_ints >= n / 1024 + 16, "short scratch");
  return pfo_iscan_launch(in, n, out, scratch, (hipStream_t)stream);
}
extern "C" int pfo_debug_mean(const float* src, int64_t n, float* out, void* stream) {
  PFO_REQUIRE(src && out && n > 0, "bad arguments");
  return pfo_mean_launch(src, n, out, (hipStream_t)stream);
}
extern "C" int pfo_debug_cq_backward(const float* const* gq, const float* const* Wq, int32_t n_layers, const float* tb, int32_t D,
                                     float* const* d_bq, float* const* d_Wq, float* d_tb, float* tb_part, const float* tb_add,
                                     const double* dtime, int32_t n_bins, float* d_tw, void* stream) {
  PFO_REQUIRE(gq && Wq && d_bq && d_Wq && tb, "null argument");
  PFO_REQUIRE(D > 0, "bad size");
  PFO_REQUIRE(n_layers >= 1 && n_layers <= PFO_MAX_LAYERS, "bad layer count");
  for (int l = 0; l < n_layers; ++l) PFO_REQUIRE(gq[l] && Wq[l] && d_bq[l] && d_Wq[l], "null layer pointer");
  PFO_REQUIRE(tb_part || d_tb, "no place for the time-bias term");
  PFO_REQUIRE(!dtime || n_bins >= 1, "bad bin count");
  return pfo_cq_backward_launch(gq, Wq, n_layers, tb, D, d_bq, d_Wq, d_tb, tb_part, tb_add, dtime, n_bins, d_tw, (hipStream_t)stream);
}
extern "C" int64_t pfo_debug_fold_parts_scratch_doubles(int32_t n) {
  if (n <= 0) { pfo_set_error("%s: bad size", __func__); return -1; }
  return pfo_fold_parts_scratch_doubles(n);
}
extern "C" int32_t pfo_debug_fold_parts_rows_in_flight(int32_t n_parts) {
  if (n_parts <= 0) { pfo_set_error("%s: bad size", __func__); return -1; }
  return pfo_fold_parts_rows_in_flight(n_parts);
}
extern "C" int pfo_debug_fold_parts(const double* parts, int32_t n_parts, int32_t n, float* out, int32_t accumulate, double* scratch,
                                    int64_t scratch_doubles, int32_t* tickets, double* out64, void* stream) {
  PFO_REQUIRE(parts && tickets && (out || out64), "null argument");
  PFO_REQUIRE(n_parts > 0 && n > 0, "bad sizes");
  PFO_REQUIRE(scratch && scratch_doubles >= pfo_fold_parts_scratch_doubles(n), "short scratch");
  return pfo_fold_parts_launch(parts, n_parts, n, out, accumulate, scratch, tickets, (hipStream_t)stream, out64);
}
