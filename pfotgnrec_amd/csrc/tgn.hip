// The TGN step as one native call per phase: pfo_tgn_forward / pfo_tgn_backward / pfo_tgn_update_state.
// Host code only: carves the caller's workspace, walks the recursion levels of
// embedding_module.py:76-175 iteratively (frontier lists instead of recursion), and queues the kernels
// on the caller's stream.  No allocation, no synchronisation, no host<->device copies.
//
// Level structure (L layers, R roots, K neighbour slots):
//   S_L = roots;  S_{l-1} = [ S_l ; neighbours(S_l) flattened ]  (|S_{l-1}| = |S_l| (1+K))
//   layer l maps features of S_{l-1} to embeddings of S_l:  x_i = H_{l-1}[i],  neighbour j of i = H_{l-1}[|S_l| + i K + j]
//   level 0 is never materialised: its rows are looked up in a per-step table of touched nodes
//   h0_tab[slot[v]] = memory'[v] + node_feat[v]   (embedding_module.py:93-98)
#include "gemm.hpp"
#include "attn.hpp"
#include "memory.hpp"
#include "explain.hpp"
#include <algorithm>
#include <math.h>
#include <string.h>
#include <stdlib.h>

int pfo_tnbr_sample_dev(const int64_t*, const int32_t*, const int32_t*, const double*, int64_t, const int32_t*, const double*,
                        int64_t, int32_t, int32_t, const int64_t*, uint64_t, uint64_t, const uint64_t*, int32_t*, int32_t*,
                        float*, float*, int32_t*, double*, int32_t*, int32_t*, void*, int32_t*, int64_t);


namespace {

struct LayerWs {
  float *QK, *attw, *ctx, *h1;             // activations kept for backward
  float* dQK;                              // layers >= 2: their own d qk' rows - their weight-gradient launch reads them on a side
                                           // stream while the caller's stream is already writing layer 1's
  float *cq, *Wqk, *cqk, *W1oT, *W1ovT;   // per-step composite weights (see the layer comment in pfo_tgn_forward)
  float *dWqk, *gqk, *dW1ovT, *dW1oT, *gq; // their gradients (per layer: the chain-back runs on the side stream)
  // layers >= 2 take the PREVIOUS layer's h1 rows as input, with that layer's fc2 (out = W2 h1 + b2) folded into their own
  // composites (see "fc2 fold" in pfo_tgn_forward): the folded weights, the two intermediates, and the gradients of all
  float *T1, *tq, *Wqk_f, *cqk_f, *W1ovT_f, *W1b_f, *b1_f;
  float *dT1, *dWqk_f, *gqk_f, *dW1ovT_f, *dW1b_f, *db1_f, *fold_slabs, *fold_vslabs;
  uint8_t* inv;
  // pre-split images of the weight operands of the large contractions (gemm.hpp PfoBimg): per step, side stream
  void *iWqk, *iWqkT, *iW1ov, *iW1ovT, *iW1b, *iW1bT, *iW2, *iW2T;
};
struct Ws {
  int32_t* nodes[PFO_MAX_LAYERS + 1];
  double* ts[PFO_MAX_LAYERS + 1];
  int32_t* eidx[PFO_MAX_LAYERS + 1];
  float* dt[PFO_MAX_LAYERS + 1];
  int32_t *mark, *slot, *touched, *n_touched, *n_core, *scan, *idx0, *winner;   // n_touched = counts[0] (all rows), n_core = counts[1]
  float *gi, *gh, *gates, *upd_mem, *h0_tab, *d_h0, *msg_rows, *h_rows;   // gi / gh: backward only (d gi / d gh)
  uint8_t* hm;
  float *cosb, *zero, *tb_part;
  void *iWih, *iWhh;
  // message MLP (msg_dim > 0): hidden activations and output of the touched rows (kept for the backward), their gradients,
  // and the weight images of the four contractions (forward W1, W2; backward W_ih^T, W2^T)
  float *mlp_hid, *mlp_out, *d_m, *d_hid;
  void *iMW1, *iMW2, *iWihT, *iMW2T;
  // layer 1 works on the touched-node table: QX[s] = h0_tab[s] [Wqk ; W1[:, E:]]^T + [cqk | 0] for every touched row s
  // (the query-side projections of all instances that sit on node s), Dq = per-row sums of the instances' gradients
  float *QX, *Dq, *dx_tab, *l1_bias;
  void* iQX;
  int32_t *seg_ptr, *seg_cur, *seg_tmp, *seg_mem, *seg_of, *seg_scratch;
  uint8_t* dqk_live;           // per layer-1 member position: does dQK row m hold a sum (attn_bwd_runs.hip)
  int32_t* cnt1;               // per layer-1 instance: entries of its node's row before its time (the run key, sampler.hip)
  LayerWs layer[PFO_MAX_LAYERS + 1];
  float *dh1, *dctx, *dQK;
  float* dH[PFO_MAX_LAYERS + 1];
  float *slabs, *slabs2, *slabs3;   // split-K slabs of the weight-gradient launches: main stream / side stream / second side stream
  double *dtime, *fold_scratch, *dtime_slab;
  int32_t* tickets;
  int64_t slab_floats;
  // cleared per step: [zero | tickets | dtime] (zero_bytes); cleared per composite build: pz = [64 zero floats | Wqk, W1ovT, cqk
  // of every layer] (pz_bytes) - in the workspace right behind the per-step region, or in the parameter cache
  size_t zero_bytes, mark_bytes;
  float* pz; size_t pz_bytes;
  bool pz_in_cache;            // pz lives in the caller's parameter cache, which the caller zeroed once (no per-build memset)
  int64_t bytes, cache_bytes;   // of the workspace / of the parameter cache (carve)
};

struct Dims {
  int L, D, Ef, H, E, C, Cp, dh, M;
  int Mg, Hm;                            // the GRU's input width (msg_dim, or M with the identity message function); msg_hidden (0 = no MLP)
  int64_t ncap[PFO_MAX_LAYERS + 1];
  int64_t capP;
};

Dims dims_of(const pfo_tgn_config* c) {
  Dims d;
  d.L = c->n_layers; d.D = c->D; d.Ef = c->Ef; d.H = c->n_heads;
  d.E = 2 * d.D; d.C = 2 * d.D + d.Ef; d.dh = d.E / d.H; d.M = 3 * d.D + d.Ef;
  d.Hm = c->msg_dim > 0 ? c->msg_hidden : 0;
  d.Mg = c->msg_dim > 0 ? c->msg_dim : d.M;
  d.Cp = (int)pfo_align_up(d.C + 2, 4);   // key columns + (sum of weights) + (valid flag), padded for 16-byte rows
  d.ncap[d.L] = c->max_roots;
  for (int l = d.L; l >= 1; --l) d.ncap[l - 1] = d.ncap[l] * (1 + (int64_t)c->max_neighbors);
  d.capP = std::min<int64_t>(c->n_nodes, d.ncap[0] + 2 * (int64_t)c->max_batch);
  return d;
}

const int64_t SLAB_FLOATS = (int64_t)(768 + 32) * 128 * 176;

template <typename T>
T* take(char*& p, int64_t count) {
  T* r = reinterpret_cast<T*>(p);
  p += pfo_align_up(count * (int64_t)sizeof(T), 256);
  return r;
}

// Two cursors: the workspace, and the parameter cache (pfo_tgn_state.pcache).  Every buffer that depends on the parameters alone
// (par) is taken from the cache when there is one - same sizes as in the workspace, which keeps its own, then unused, copies.
struct Carver {
  char *p, *q;
  bool cached;
  template <typename T> T* ws(int64_t count) { return take<T>(p, count); }
  template <typename T> T* par(int64_t count) { T* r = take<T>(p, count); return cached ? take<T>(q, count) : r; }
};

// layer l's part of the workspace (and of the parameter cache)
void carve_layer(Carver& k, const Dims& d, int l, int64_t Km, Ws& w) {
  const int64_t N = d.ncap[l], HCp = (int64_t)d.H * d.Cp, HCpD = HCp * d.D, DD = (int64_t)d.D * d.D, ED = (int64_t)d.E * d.D;
  LayerWs& lw = w.layer[l];
  lw.cq = k.par<float>(d.E);     lw.W1oT = k.par<float>(ED);
  lw.dWqk = k.ws<float>(HCpD);   lw.gqk = k.ws<float>(HCp);
  lw.dW1ovT = k.ws<float>(HCpD); lw.dW1oT = k.ws<float>(ED);    lw.gq = k.ws<float>(d.E);
  lw.iWqk = k.par<char>(pfo_bimg_bytes(HCp, d.D));   lw.iWqkT = k.par<char>(pfo_bimg_bytes(d.D, HCp));
  lw.iW1ovT = k.par<char>(pfo_bimg_bytes(HCp, d.D)); lw.iW1ov = k.par<char>(pfo_bimg_bytes(d.D, HCp));
  lw.iW1b = k.par<char>(pfo_bimg_bytes(d.D, d.D));   lw.iW1bT = k.par<char>(pfo_bimg_bytes(d.D, d.D));
  lw.iW2 = k.par<char>(pfo_bimg_bytes(d.D, d.D));    lw.iW2T = k.par<char>(pfo_bimg_bytes(d.D, d.D));
  lw.QK = l > 1 ? k.ws<float>(N * HCp) : nullptr;      // layer 1 reads its rows from the touched-node table QX
  lw.attw = k.ws<float>(N * d.H * Km);
  lw.inv = k.ws<uint8_t>(N);
  lw.ctx = k.ws<float>(N * HCp);
  lw.h1 = k.ws<float>(N * d.D);
  if (l < d.L) w.dH[l] = k.ws<float>(N * d.D);
  if (l < 2) return;
  lw.dQK = k.ws<float>(N * HCp);
  lw.T1 = k.par<float>(HCpD);      lw.tq = k.par<float>(HCp);
  lw.Wqk_f = k.par<float>(HCpD);   lw.cqk_f = k.par<float>(HCp);
  lw.W1ovT_f = k.par<float>(HCpD); lw.W1b_f = k.par<float>(DD);   lw.b1_f = k.par<float>(d.D);
  lw.dT1 = k.ws<float>(HCpD);
  lw.dWqk_f = k.ws<float>(HCpD);   lw.gqk_f = k.ws<float>(HCp);
  lw.dW1ovT_f = k.ws<float>(HCpD); lw.dW1b_f = k.ws<float>(DD);   lw.db1_f = k.ws<float>(d.D);
  lw.fold_slabs = k.ws<float>((2 * d.H + 2) * DD);
  lw.fold_vslabs = k.ws<float>((int64_t)(d.H + 2) * d.D);
}

// (`cached` and not `cache != nullptr`: the size queries carve from null bases)
Ws carve(const pfo_tgn_config* c, void* base, void* cache = nullptr, bool cached = false) {
  const Dims d = dims_of(c);
  Ws w;
  memset(&w, 0, sizeof(w));
  Carver k = {reinterpret_cast<char*>(base), reinterpret_cast<char*>(cache), cached};
  char*& p = k.p;
  const int64_t Km = c->max_neighbors;
  for (int l = 0; l <= d.L; ++l) {
    w.nodes[l] = k.ws<int32_t>(d.ncap[l]);
    if (l >= 1) {
      w.ts[l] = k.ws<double>(d.ncap[l]);
      w.eidx[l] = k.ws<int32_t>(d.ncap[l] * Km);
      w.dt[l] = k.ws<float>(d.ncap[l] * Km);
    }
  }
  // one memset per step clears [zero | tickets | dtime]; a composite build clears pz = [64 floats | Wqk, W1ovT, cqk of every
  // layer] (padding rows / columns of the composites must be zero; with a parameter cache pz lives there)
  w.zero = k.ws<float>(64);
  w.tickets = k.ws<int32_t>(64);
  w.dtime = k.ws<double>((int64_t)pfo_attn_bwd_max_parts() * 2 * d.D);      // time-encoder gradient bins, also cleared per step
  w.zero_bytes = (size_t)(p - reinterpret_cast<char*>(w.zero));
  w.pz = k.par<float>(64);
  for (int l = 1; l <= d.L; ++l) {
    LayerWs& lw = w.layer[l];
    lw.Wqk = k.par<float>((int64_t)d.H * d.Cp * d.D);
    lw.W1ovT = k.par<float>((int64_t)d.H * d.Cp * d.D);
    // layer 1: cqk is the head of the bias of the stacked [Wqk ; W1[:, E:]] projection; its tail (D floats) stays zero
    lw.cqk = k.par<float>((int64_t)d.H * d.Cp + (l == 1 ? d.D : 0));
  }
  w.l1_bias = w.layer[1].cqk;
  w.pz_bytes = (size_t)((cached ? k.q : p) - reinterpret_cast<char*>(w.pz));
  w.pz_in_cache = cached;
  w.cosb = k.par<float>(d.D);
  w.tb_part = k.ws<float>(d.D);
  {
    const int WQ = d.H * d.Cp + d.D;
    // one memset per step clears [touched-node flags | block flags of the one-pass compaction]
    w.mark = k.ws<int32_t>(c->n_nodes);
    w.scan = k.ws<int32_t>(pfo_compact_scratch_ints(c->n_nodes));
    w.mark_bytes = (size_t)(p - reinterpret_cast<char*>(w.mark));
    w.slot = k.ws<int32_t>(c->n_nodes);
    w.touched = k.ws<int32_t>(d.capP);
    w.n_touched = k.ws<int32_t>(64);
    w.n_core = w.n_touched + 1;
    w.idx0 = k.ws<int32_t>(d.ncap[0]);
    w.h0_tab = k.ws<float>(d.capP * d.D);
    w.QX = k.ws<float>(d.capP * WQ);
    w.Dq = k.ws<float>(d.capP * WQ);
    w.dx_tab = k.ws<float>(d.capP * d.D);
    w.iQX = k.par<char>(pfo_bimg_bytes(WQ, d.D));
    w.seg_ptr = k.ws<int32_t>(d.capP + 1);
    w.seg_cur = k.ws<int32_t>(d.capP + 1);
    w.seg_tmp = k.ws<int32_t>(d.ncap[1]);
    w.seg_mem = k.ws<int32_t>(d.ncap[1]);
    w.seg_of = k.ws<int32_t>(pfo_seg_of_ints(d.ncap[1]));
    w.seg_scratch = k.ws<int32_t>(pfo_seg_scratch_ints((int)d.capP));
    w.cnt1 = k.ws<int32_t>(d.ncap[1]);
    w.dqk_live = k.ws<uint8_t>(d.ncap[1]);
  }
  if (c->use_memory) {
    w.winner = k.ws<int32_t>(c->n_nodes);
    w.gi = k.ws<float>(d.capP * 3 * d.D);
    w.gh = k.ws<float>(d.capP * 3 * d.D);
    w.gates = k.ws<float>(d.capP * 4 * d.D);
    w.upd_mem = k.ws<float>(d.capP * d.D);
    w.d_h0 = k.ws<float>(PFO_GRAD_REPLICAS * d.capP * d.D);     // one replica per XCD (attn_bwd.hip, DMODE 1)
    w.msg_rows = k.ws<float>(d.capP * d.M);
    w.h_rows = k.ws<float>(d.capP * d.D);
    w.hm = k.ws<uint8_t>(d.capP);
    w.iWih = k.par<char>(pfo_gru_img_bytes(d.D, d.Mg));
    w.iWhh = k.par<char>(pfo_gru_img_bytes(d.D, d.D));
    if (d.Hm > 0) {
      w.mlp_hid = k.ws<float>(d.capP * d.Hm);
      w.mlp_out = k.ws<float>(d.capP * d.Mg);
      w.d_m = k.ws<float>(d.capP * d.Mg);
      w.d_hid = k.ws<float>(d.capP * d.Hm);
      w.iMW1 = k.par<char>(pfo_bimg_bytes(d.Hm, d.M));
      w.iMW2 = k.par<char>(pfo_bimg_bytes(d.Mg, d.Hm));
      w.iWihT = k.par<char>(pfo_bimg_bytes(d.Mg, 3 * d.D));
      w.iMW2T = k.par<char>(pfo_bimg_bytes(d.Hm, d.Mg));
    }
  }
  for (int l = 1; l <= d.L; ++l) carve_layer(k, d, l, Km, w);
  const int64_t N1 = d.ncap[1];
  w.dh1 = k.ws<float>(N1 * d.D);
  w.dctx = k.ws<float>(N1 * d.H * d.Cp);
  w.dQK = k.ws<float>(N1 * d.H * d.Cp);
  w.slab_floats = SLAB_FLOATS;
  w.slabs = k.ws<float>(w.slab_floats);
  w.slabs2 = k.ws<float>(w.slab_floats);
  w.slabs3 = k.ws<float>(w.slab_floats);
  w.fold_scratch = k.ws<double>(pfo_fold_parts_scratch_doubles(2 * d.D));
  {
    // deterministic mode: one slab row of time-encoder partials per attention-backward workgroup, all layers
    int64_t rows = 0;
    for (int l = 1; l <= d.L; ++l) rows += pfo_attn_bwd_det_parts(d.ncap[l]);
    w.dtime_slab = k.ws<double>(rows * 2 * d.D);
  }
  w.bytes = p - reinterpret_cast<char*>(base);
  w.cache_bytes = k.q - reinterpret_cast<char*>(cache);
  return w;
}

int check_cfg(const pfo_tgn_config* c) {
  PFO_REQUIRE(c != nullptr, "null config");
  PFO_REQUIRE(c->n_layers >= 1 && c->n_layers <= PFO_MAX_LAYERS, "n_layers must be in [1, 4]");
  PFO_REQUIRE(c->D >= 4 && c->D <= 256 && (c->D % 4) == 0, "D must be a multiple of 4 in [4, 256]");
  PFO_REQUIRE(c->Ef >= 0 && c->Ef <= 64 && (c->Ef % 4) == 0, "Ef must be a multiple of 4 in [0, 64]");
  PFO_REQUIRE(c->n_heads == 1 || c->n_heads == 2 || c->n_heads == 4, "n_heads must be 1, 2 or 4");
  PFO_REQUIRE(((2 * c->D) % c->n_heads) == 0, "n_heads must divide 2D");
  PFO_REQUIRE(c->max_batch >= 0, "bad max_batch");
  PFO_REQUIRE(c->n_nodes >= 2 && c->n_edges_p1 >= 1, "bad graph sizes");
  PFO_REQUIRE(c->max_roots >= 1 && c->max_neighbors >= 1 && c->max_neighbors <= PFO_MAX_NEIGHBORS, "bad capacities");
  PFO_REQUIRE(c->msg_dim >= 0 && c->msg_dim <= 4096 && (c->msg_dim % 4) == 0, "msg_dim must be a multiple of 4 in [0, 4096]");
  PFO_REQUIRE(c->msg_dim == 0 || c->use_memory, "the MLP message function needs use_memory");
  PFO_REQUIRE(c->msg_dim == 0 || (c->msg_hidden >= 1 && c->msg_hidden <= 4096), "msg_hidden must be in [1, 4096] with the MLP message function");
  return PFO_OK;
}

struct Params {
  const float *tw, *tb, *w_ih, *w_hh, *b_ih, *b_hh;
  const float *m_w1, *m_b1, *m_w2, *m_b2;
  struct { const float *wq, *wk, *wv, *b_in, *wo, *bo, *w1, *b1, *w2, *b2; } l[PFO_MAX_LAYERS + 1];
};
struct Grads {
  float *tw, *tb, *w_ih, *w_hh, *b_ih, *b_hh;
  float *m_w1, *m_b1, *m_w2, *m_b2;
  struct { float *wq, *wk, *wv, *b_in, *wo, *bo, *w1, *b1, *w2, *b2; } l[PFO_MAX_LAYERS + 1];
};

template <typename PT, typename FT>
void bind(const pfo_tgn_layout& lay, FT* base, PT& p, int L, bool mem) {
  p.tw = base + lay.time_w; p.tb = base + lay.time_b;
  if (mem) {
    p.w_ih = base + lay.gru_w_ih; p.w_hh = base + lay.gru_w_hh; p.b_ih = base + lay.gru_b_ih; p.b_hh = base + lay.gru_b_hh;
  } else {
    p.w_ih = p.w_hh = p.b_ih = p.b_hh = nullptr;
  }
  const bool mlp = mem && lay.mlp_w1 >= 0;
  p.m_w1 = mlp ? base + lay.mlp_w1 : nullptr; p.m_b1 = mlp ? base + lay.mlp_b1 : nullptr;
  p.m_w2 = mlp ? base + lay.mlp_w2 : nullptr; p.m_b2 = mlp ? base + lay.mlp_b2 : nullptr;
  for (int l = 1; l <= L; ++l) {
    const pfo_tgn_layer_layout& q = lay.layer[l - 1];
    p.l[l].wq = base + q.wq; p.l[l].wk = base + q.wk; p.l[l].wv = base + q.wv; p.l[l].b_in = base + q.b_in;
    p.l[l].wo = base + q.wo; p.l[l].bo = base + q.bo; p.l[l].w1 = base + q.w1; p.l[l].b1 = base + q.b1;
    p.l[l].w2 = base + q.w2; p.l[l].b2 = base + q.b2;
  }
}

// plain C = A[M,K] * B[N,K]^T (+bias)
PfoGemm g_nt(const float* A, int64_t lda, const int32_t* a_idx, const float* B, int64_t ldb, float* C, int64_t ldc, int M,
             int N, int K, const float* bias) {
  PfoGemm g;
  g.A[0] = A; g.lda[0] = lda; g.a_idx[0] = a_idx; g.B[0] = B; g.ldb[0] = ldb; g.K[0] = K;
  g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.bias = bias;
  return g;
}
// C = A[M,K] * B[K,N]
PfoGemm g_nn(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int M, int N, int K) {
  PfoGemm g = g_nt(A, lda, nullptr, B, ldb, C, ldc, M, N, K, nullptr);
  g.b_kmajor = 1;
  return g;
}
#define PFO_MAX_DEVICES 16
// Internal side stream: the composite-weight products (forward) and their gradient chain (backward) are tiny
// dependent launches; they run beside the main stream's work and are joined by events where their results are needed.
struct Side {
  hipStream_t s = nullptr, s2 = nullptr;
  hipEvent_t tn_a_done = nullptr, done2 = nullptr, gru_done = nullptr, comp_done = nullptr, pc_a = nullptr, pc_b = nullptr;
  hipEvent_t main_done = nullptr, side_done = nullptr;
  // Deferred work on `s` (a backward end, the optimizer step behind it: pfo_tgn_batch.defer_join) is counted in GENERATIONS:
  // side_gen grows when work is queued there, every joining stream remembers the generation it last waited for.  (One
  // "pending" flag that the first joiner cleared let a prepare call on the prefetch stream consume the join: tgn.join(),
  // state_dict() and the next backward on the caller's stream then read parameters the side stream was still writing.)
  uint64_t side_gen = 0, recorded_gen = 0;
  bool last_backward_deferred = false;                           // pfo_tgn_adam_side may only follow such a backward
  hipStream_t deferred_from = nullptr;                           // the caller's stream of that backward (the only stream the side stream is already ordered behind)
  // Buckets of a side-stream optimizer step in order of FIRST USE (pfo_tgn_adam_side_bucket): early_done fires behind the
  // kernel that finishes the parameters the next forward reads on the caller's stream (time encoder, GRU, layer 1's biases);
  // it stands for the whole side stream as long as nothing but later buckets of the same step was queued behind it.
  hipEvent_t early_done = nullptr;
  uint64_t early_gen = 0;
  bool early_ok = false;
  struct Joined { hipStream_t s; uint64_t gen; } joined[8] = {};
  int n_joined = 0;
  bool pending_for(hipStream_t s) const {
    if (side_gen == 0) return false;
    for (int i = 0; i < n_joined; ++i) if (joined[i].s == s) return joined[i].gen != side_gen;
    return true;
  }
  void mark_joined(hipStream_t s) {
    for (int i = 0; i < n_joined; ++i) if (joined[i].s == s) { joined[i].gen = side_gen; return; }
    if (n_joined < 8) { joined[n_joined].s = s; joined[n_joined].gen = side_gen; ++n_joined; return; }
    for (int i = 1; i < 8; ++i) joined[i - 1] = joined[i];       // more streams than slots: the oldest entry goes (it will wait again)
    joined[7].s = s; joined[7].gen = side_gen;
  }
  hipEvent_t fork = nullptr, done = nullptr, seg_done = nullptr, tn_a = nullptr, tn_b = nullptr, fold_done = nullptr;
  hipEvent_t layer[PFO_MAX_LAYERS + 1] = {};
  bool ok = false;
};
Side& side() {
  // one set per device (streams and events belong to the device that was current when they were made)
  static Side sds[PFO_MAX_DEVICES];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= PFO_MAX_DEVICES) dev = 0;
  Side& sd = sds[dev];
  if (!sd.ok) {
    // The side streams live in the HIGH and the LOW priority class: the runtime multiplexes all streams of a process onto
    // GPU_MAX_HW_QUEUES hardware queues (default 4) PER PRIORITY CLASS, and once a process holds more streams than that (a
    // process group: RCCL, c10d) a normal-priority side stream shares a hardware queue with the caller's stream - every
    // "beside" of this file silently becomes "behind" (rank path at world 1 on RCCL: 1.65 ms per step against 1.39).  In
    // classes of their own they cannot.  (Dispatch priority itself changes nothing measurable: round 3.)
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);           // lo = least (numerically largest), hi = greatest
    bool good = hipStreamCreateWithPriority(&sd.s, hipStreamNonBlocking, hi) == hipSuccess;
    good = good && hipStreamCreateWithPriority(&sd.s2, hipStreamNonBlocking, lo) == hipSuccess;
    hipEvent_t* const evs[] = {&sd.tn_a_done, &sd.done2, &sd.fork, &sd.done, &sd.seg_done, &sd.tn_a, &sd.tn_b, &sd.fold_done,
                               &sd.gru_done, &sd.comp_done, &sd.pc_a, &sd.pc_b, &sd.main_done, &sd.side_done, &sd.early_done};
    for (hipEvent_t* e : evs) good = good && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
    for (int l = 0; l <= PFO_MAX_LAYERS; ++l) good = good && hipEventCreateWithFlags(&sd.layer[l], hipEventDisableTiming) == hipSuccess;
    sd.ok = good;
  }
  return sd;
}
#define HIPOK(expr, msg) PFO_REQUIRE((expr) == hipSuccess, msg)
// `s` waits for whatever a deferred backward end / side-stream optimizer step left in flight (pfo_tgn_batch.defer_join)
// allow_early (pfo_tgn_forward only): when the side stream's tail is a bucketed optimizer step, the caller's stream waits for
// the first-use bucket alone and is NOT marked joined - everything else the forward takes from the side streams arrives
// through events recorded there behind the later buckets (composite weights, weight images, the fc2 fold), and the next full
// join (the backward's) still waits for all of it.
int side_join(Side& sd, hipStream_t s, bool allow_early = false) {
  if (!sd.pending_for(s)) return PFO_OK;
  if (allow_early && sd.early_ok && sd.early_gen == sd.side_gen) {
    hipStreamCaptureStatus cap0 = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap0) == hipSuccess && cap0 == hipStreamCaptureStatusNone) {
      HIPOK(hipStreamWaitEvent(s, sd.early_done, 0), "event wait failed");
      return PFO_OK;
    }
  }
  // A capturing stream does not join: a capture starts from a synchronised device (torch.cuda.graph, GraphedTrainStep.capture),
  // so nothing deferred is still in flight, and the calls below would be captured - by the time a forward joins, the side stream
  // belongs to the capture (it waited for the fork event), a record on it would turn side_done into a capture-only event and
  // every later plain wait on it would fail.  (A backward under capture never defers its end: pfo_tgn_backward_ev.)
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) { sd.mark_joined(s); return PFO_OK; }
  if (sd.recorded_gen != sd.side_gen) {                          // one record per generation, shared by every joiner
    HIPOK(hipEventRecord(sd.side_done, sd.s), "event record failed");
    sd.recorded_gen = sd.side_gen;
  }
  HIPOK(hipStreamWaitEvent(s, sd.side_done, 0), "event wait failed");
  sd.mark_joined(s);
  return PFO_OK;
}

#define RUN(expr)                  \
  do {                             \
    int rc__ = (expr);             \
    if (rc__ != PFO_OK) return rc__; \
  } while (0)

}  // namespace

// =============================================================================================
extern "C" int pfo_tgn_param_layout(const pfo_tgn_config* c, pfo_tgn_layout* out) {
  if (int rc = check_cfg(c)) return rc;
  PFO_REQUIRE(out != nullptr, "null output");
  const Dims d = dims_of(c);
  int64_t o = 0;
  auto put = [&](int64_t n) { int64_t r = o; o += n; return r; };
  memset(out, 0, sizeof(*out));
  out->time_w = put(d.D);
  out->time_b = put(d.D);
  if (c->use_memory) {
    out->gru_w_ih = put((int64_t)3 * d.D * d.Mg);
    out->gru_w_hh = put((int64_t)3 * d.D * d.D);
    out->gru_b_ih = put(3 * d.D);
    out->gru_b_hh = put(3 * d.D);
  } else {
    out->gru_w_ih = out->gru_w_hh = out->gru_b_ih = out->gru_b_hh = -1;
  }
  out->mlp_w1 = out->mlp_b1 = out->mlp_w2 = out->mlp_b2 = -1;
  if (d.Hm > 0) {
    // behind the GRU's block, not at the end: its gradients finish last, with the GRU's (pfo_tgn_grad_split).  Every tensor
    // starts at a multiple of 4 floats (msg_hidden may be odd), and so does what follows the block
    auto put4 = [&](int64_t n) { o = pfo_align_up(o, 4); return put(n); };
    out->mlp_w1 = put4((int64_t)d.Hm * d.M);
    out->mlp_b1 = put4(d.Hm);
    out->mlp_w2 = put4((int64_t)d.Mg * d.Hm);
    out->mlp_b2 = put4(d.Mg);
    o = pfo_align_up(o, 4);
  }
  for (int l = 0; l < d.L; ++l) {
    pfo_tgn_layer_layout& q = out->layer[l];
    q.wq = put((int64_t)d.E * d.E);
    q.wk = put((int64_t)d.E * d.C);
    q.wv = put((int64_t)d.E * d.C);
    q.b_in = put(3 * d.E);
    q.wo = put((int64_t)d.E * d.E);
    q.bo = put(d.E);
    q.w1 = put((int64_t)d.D * (d.E + d.D));
    q.b1 = put(d.D);
    q.w2 = put((int64_t)d.D * d.D);
    q.b2 = put(d.D);
  }
  out->total = o;
  return PFO_OK;
}

extern "C" int64_t pfo_tgn_workspace_bytes(const pfo_tgn_config* c) {
  if (check_cfg(c) != PFO_OK) return -1;
  return carve(c, nullptr).bytes + 256;
}

extern "C" int pfo_tgn_debug_views(const pfo_tgn_config* c, void* workspace, pfo_tgn_debug* out) {
  if (int rc = check_cfg(c)) return rc;
  PFO_REQUIRE(workspace && out, "null argument");
  const Ws w = carve(c, workspace);
  out->n_touched = w.n_touched; out->touched_ids = w.touched; out->h0_table = w.h0_tab; out->slot = w.slot;
  const Dims d = dims_of(c);
  out->n_core = w.n_core;
  out->l1_ctx = w.layer[1].ctx;
  out->l1_dh1 = d.L == 1 ? w.dh1 : w.dH[1];       // the top layer writes dh1 itself, below it the layer above does
  out->l1_dW1ovT = w.layer[1].dW1ovT;
  out->gru_dgi = c->use_memory ? w.gi : nullptr;
  out->gru_msg_rows = c->use_memory ? w.msg_rows : nullptr;
  out->Cp = d.Cp;
  out->mlp_hid = w.mlp_hid; out->mlp_out = w.mlp_out;
  return PFO_OK;
}

// The explanation query reads what a forward left in its workspace (include/pfotgn.h): level L's tables for the roots, level
// L - 1's for their neighbours' instances (rows R .. R + R K).  Level l's neighbour ids sit behind the n_l nodes of nodes[l - 1].
// (a weak reference: this file also links host-only, without the kernels' objects - tests/host/step_trace.cpp)
int pfo_explain_launch(const PfoExplain& a, hipStream_t s) __attribute__((weak));
extern "C" int pfo_tgn_explain(const pfo_tgn_config* c, const void* workspace, int32_t R, int32_t K, int32_t hops, int32_t m,
                               int32_t* node_out, double* weight_out, int32_t* n_valid_out, int32_t* count_out, float* age_out,
                               int32_t* eidx_out, int32_t* raw_nbr, float* raw_w, float* raw_dt, int32_t* raw_eidx,
                               int32_t* raw_nbr2, float* raw_w2, float* raw_dt2, int32_t* raw_eidx2, void* stream) {
  if (int rc = check_cfg(c)) return rc;
  PFO_REQUIRE(m >= 1 && m <= PFO_EXPLAIN_MAX_WIDTH, "m must lie in [1, PFO_EXPLAIN_MAX_WIDTH]");
  PFO_REQUIRE(hops >= 1 && hops <= std::min(2, c->n_layers), "hops must lie in [1, min(2, n_layers)]");
  PFO_REQUIRE(K >= 1 && K <= PFO_MAX_NEIGHBORS && K <= c->max_neighbors, "K must lie in [1, min(PFO_MAX_NEIGHBORS, max_neighbors)]");
  PFO_REQUIRE(R >= 0 && R <= c->max_roots, "R must lie in [0, max_roots]");
  if (R == 0) return PFO_OK;
  PFO_REQUIRE(workspace && node_out && weight_out && n_valid_out && count_out && age_out && eidx_out, "null pointer");
  const int n_raw = (raw_nbr != nullptr) + (raw_w != nullptr) + (raw_dt != nullptr) + (raw_eidx != nullptr);
  const int n_raw2 = (raw_nbr2 != nullptr) + (raw_w2 != nullptr) + (raw_dt2 != nullptr) + (raw_eidx2 != nullptr);
  PFO_REQUIRE((n_raw == 0 || n_raw == 4) && (n_raw2 == 0 || n_raw2 == 4), "null pointer: a raw group is given whole or not at all");
  PFO_REQUIRE(&pfo_explain_launch != nullptr, "built without csrc/explain.hip");
  const Ws w = carve(c, const_cast<void*>(workspace));
  const int L = c->n_layers, H = c->n_heads;
  PfoExplain a;
  memset(&a, 0, sizeof(a));
  a.R = R; a.K = K; a.H = H; a.hops = hops; a.m = m;
  a.nbr = w.nodes[L - 1] + R; a.attw = w.layer[L].attw; a.dt = w.dt[L]; a.eidx = w.eidx[L];
  if (hops == 2) {
    const int64_t n_below = (int64_t)R * (1 + K), skip = (int64_t)R * K;     // level L - 1: its R self rows come first
    a.nbr2 = w.nodes[L - 2] + n_below + skip; a.attw2 = w.layer[L - 1].attw + skip * H;
    a.dt2 = w.dt[L - 1] + skip; a.eidx2 = w.eidx[L - 1] + skip;
    a.raw_nbr2 = raw_nbr2; a.raw_w2 = raw_w2; a.raw_dt2 = raw_dt2; a.raw_eidx2 = raw_eidx2;
  }
  a.node_out = node_out; a.weight_out = weight_out; a.n_valid_out = n_valid_out; a.count_out = count_out; a.age_out = age_out;
  a.eidx_out = eidx_out;
  a.raw_nbr = raw_nbr; a.raw_w = raw_w; a.raw_dt = raw_dt; a.raw_eidx = raw_eidx;
  return pfo_explain_launch(a, (hipStream_t)stream);
}

static int level_sizes(const pfo_tgn_config* c, const pfo_tgn_batch* b, int64_t* n) {
  PFO_REQUIRE(b != nullptr, "null batch");
  PFO_REQUIRE(b->R >= 1 && b->R <= c->max_roots, "R exceeds the workspace capacity (max_roots)");
  PFO_REQUIRE(b->K >= 1 && b->K <= c->max_neighbors, "K exceeds the workspace capacity (max_neighbors)");
  n[c->n_layers] = b->R;
  for (int l = c->n_layers; l >= 1; --l) n[l - 1] = n[l] * (1 + (int64_t)b->K);
  PFO_REQUIRE(n[0] < (int64_t)1 << 31, "too many level-0 references");
  return PFO_OK;
}
// the batch arguments pfo_tgn_prepare and pfo_tgn_forward both read
static int check_batch(const pfo_tgn_config* c, const pfo_tgn_batch* b) {
  PFO_REQUIRE(b->roots && b->root_ts, "null batch arrays");
  PFO_REQUIRE(b->uniform >= 0 && b->uniform <= 2, "bad sampling mode");
  PFO_REQUIRE(b->uniform != 1 || b->draws, "mode 1 needs draws");
  PFO_REQUIRE(b->n_extra >= 0 && b->n_extra <= 2 * c->max_batch, "n_extra exceeds 2 * max_batch");
  PFO_REQUIRE(b->n_extra == 0 || b->extra_nodes, "null extra_nodes");
  return PFO_OK;
}

// Replicas of the level-0 gradient table the layer-1 attention backward adds into: per-XCD replicas pay off only for the
// per-instance atomics (uniform sampling: 4 replicas 0.537 -> 0.506 ms); the run-merged kernel issues 2-3x fewer and measures
// best on ONE table (1.656 vs 1.665 ms/step); the deterministic int64 table is always one
static int grad_replicas(const pfo_tgn_config* c, const pfo_tgn_batch* b) {
  const int det = b->deterministic ? 1 : 0;
  return (det || (c->use_memory && !b->uniform && pfo_attn_bwd_runs_possible(b->K, c->D, c->n_heads))) ? 1 : PFO_GRAD_REPLICAS;
}
static_assert(PFO_GRAD_REPLICAS >= 2, "the deterministic int64 gradient table needs the room of two float replicas");

// ---- One call's context: everything pfo_tgn_prepare / pfo_tgn_forward / pfo_tgn_backward_ev derive from their arguments
// before they queue anything (open_step), then what the stages of one call hand to each other.
namespace {
struct Step {
  explicit Step(Side& sd_) : sd(sd_) {}
  const pfo_tgn_config* c = nullptr; const pfo_tgn_state* st = nullptr; const pfo_tgn_batch* b = nullptr;
  int64_t n[PFO_MAX_LAYERS + 1] = {};   // rows per level of this batch
  Dims d;
  Ws w;                                 // (parameter-only buffers in the state's parameter cache, if it has one)
  pfo_tgn_layout lay;
  Params P; Grads G;                    // (G: backward only)
  Side& sd;
  hipStream_t s = nullptr, ss = nullptr, s2 = nullptr;   // the caller's stream, the library's two side streams
  int capP = 0;                         // rows of this batch's touched-node table, at most
  int det = 0, n_rep = 1;               // deterministic backward; replicas of the level-0 gradient table (grad_replicas)
  int64_t rep_stride = 0;               // floats between the per-XCD replicas of d_h0
  float scale = 1.f;
  // The capture status of the caller's stream, asked ONCE per call (nothing inside a call begins or ends a capture there).
  // Not capturing: events are bound to launches (common.hpp), pc_a / pc_b are waited for, the backward joins in a chain.
  bool capturing = false;
  bool build = false, pack_side = false, fused_state = false;      // forward
  const float* d_emb = nullptr; void* top_ready_event = nullptr;   // backward, from here on
  bool seg_fwd = false;                 // the forward queued seg_prologue (pfo_tgn_batch.seg_in_forward)
  const float* mean_src = nullptr; int64_t mean_n = 0; float* mean_out = nullptr;   // the loss mean the caller left to this call
  int64_t det_rows = 0;                 // slab rows written so far (deterministic mode)
};
}  // namespace
// (each entry first checks the arguments only it takes; `st` is non-null here)
static int open_step(Step& S, const pfo_tgn_config* c, const pfo_tgn_state* st, const pfo_tgn_batch* b, void* workspace, void* stream) {
  S.c = c; S.st = st; S.b = b;
  RUN(level_sizes(c, b, S.n));
  S.d = dims_of(c);
  S.w = carve(c, workspace, st->pcache, st->pcache != nullptr);   // parameter-only buffers live in the caller's cache
  RUN(pfo_tgn_param_layout(c, &S.lay));
  if (st->params) bind(S.lay, st->params, S.P, S.d.L, c->use_memory != 0);
  S.s = (hipStream_t)stream; S.ss = S.sd.s; S.s2 = S.sd.s2;
  S.capP = (int)std::min<int64_t>(c->n_nodes, S.n[0] + b->n_extra);
  S.det = b->deterministic ? 1 : 0;
  S.n_rep = grad_replicas(c, b);
  S.rep_stride = (int64_t)S.d.capP * S.d.D;
  S.scale = 1.0f / sqrtf((float)S.d.dh);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(S.s, &cap) != hipSuccess) cap = hipStreamCaptureStatusActive;
  S.capturing = cap != hipStreamCaptureStatusNone;
  return PFO_OK;
}

// One table for the per-layer names of ranges (rocprofv3 --marker-trace) and marks (pfo_marks_*)
enum { NM_FWD, NM_QK, NM_AT, NM_H1, NM_BWD, NM_DH1, NM_DCTX, NM_BATTN, NM_DX, NM_KINDS };
#define PFO_L4(a, z) {"", a "1" z, a "2" z, a "3" z, a "4" z}
static const char* const LAYER_NAMES[NM_KINDS][PFO_MAX_LAYERS + 1] = {
    PFO_L4("forward layer ", ""), PFO_L4("fwd.L", ".qk"), PFO_L4("fwd.L", ".attn"), PFO_L4("fwd.L", ".h1"),
    PFO_L4("backward layer ", ""), PFO_L4("bwd.L", ".dh1"), PFO_L4("bwd.L", ".dctx"), PFO_L4("bwd.L", ".attn"),
    {"", "bwd.L1.dx_tab", "bwd.L2.dx", "bwd.L3.dx", "bwd.L4.dx"}};

// What layer l reads and writes, forward and backward.  Layer 1 works on rows of the touched-node table; layers >= 2 read the
// previous layer's h1 rows through their fc2-folded composites (build_stage_b, "fc2 fold"): backward, their weight gradients
// land in the folded composites' gradient buffers and are unfolded on the side stream (unfold_fc2).
namespace {
struct LayerView {
  int l, N; bool folded; const LayerWs* lw;
  const float* xA; const int32_t* x_idx;
  const float *Wqk, *cqk, *W1ovT, *W1b, *b1; int64_t W1b_ld;
  float *dx, *dqk, *dWqk, *gqk, *dW1ovT;
};
}  // namespace
static LayerView layer_view(const Step& S, int l) {
  const Ws& w = S.w;
  const LayerWs& lw = w.layer[l];
  const int D = S.d.D, E = S.d.E;
  LayerView v;
  v.l = l; v.N = (int)S.n[l]; v.folded = l >= 2; v.lw = &lw;
  v.xA = v.folded ? w.layer[l - 1].h1 : w.h0_tab;
  v.x_idx = v.folded ? nullptr : w.idx0;
  v.Wqk = v.folded ? lw.Wqk_f : lw.Wqk;
  v.cqk = v.folded ? lw.cqk_f : lw.cqk;
  v.W1ovT = v.folded ? lw.W1ovT_f : lw.W1ovT;
  v.W1b = v.folded ? lw.W1b_f : S.P.l[l].w1 + E;
  v.W1b_ld = v.folded ? D : E + D;
  v.b1 = v.folded ? lw.b1_f : S.P.l[l].b1;
  v.dx = v.folded ? w.dH[l - 1] : nullptr;                  // rows [0, N) of the previous level's gradient
  v.dqk = v.folded ? lw.dQK : w.dQK;
  v.dWqk = v.folded ? lw.dWqk_f : lw.dWqk;
  v.gqk = v.folded ? lw.gqk_f : lw.gqk;
  v.dW1ovT = v.folded ? lw.dW1ovT_f : lw.dW1ovT;
  return v;
}
// the attention launch of layer l as forward and backward both describe it (the backward adds its own fields on top)
static PfoAttn attn_of(const Step& S, const LayerView& v) {
  const Ws& w = S.w;
  const pfo_tgn_batch* b = S.b;
  const int l = v.l, N = v.N, HCp = S.d.H * S.d.Cp;
  PfoAttn a;
  a.N = N; a.K = b->K; a.D = S.d.D; a.Ef = S.d.Ef; a.H = S.d.H; a.Cp = S.d.Cp;
  a.QK = (l == 1) ? w.QX : v.lw->QK; a.qk_row = (l == 1) ? w.idx0 : nullptr; a.qk_ld = (l == 1) ? HCp + S.d.D : HCp;
  a.nbr_tab = v.xA; a.nbr_ld = S.d.D;
  a.nbr_rows = (l == 1) ? S.capP : S.n[l - 1]; a.edge_rows = S.c->n_edges_p1;
  a.nbr_row = (l == 1) ? w.idx0 + N : nullptr;
  a.nbr_row_base = N;
  a.nbr_ids = w.nodes[l - 1] + N;
  a.edge_feat = S.st->edge_feat; a.eidx = w.eidx[l]; a.dt = w.dt[l]; a.tw = S.P.tw; a.tb = S.P.tb;
  a.scale = S.scale; a.dropout_p = b->dropout_p; a.seed = b->seed; a.offset = b->offset + 0x51ED0000ull + (uint64_t)l; a.offset_dev = b->offset_dev;
  a.keep_inject = (b->dropout_keep && b->training) ? b->dropout_keep[S.d.L - l] : nullptr;
  a.ctx = v.lw->ctx; a.attw = v.lw->attw; a.inv = v.lw->inv;
  return a;
}

// What the backward's layer-1 kernels need and that depends on the sampled levels alone: the cleared level-0 gradient rows and
// the layer-1 instances grouped by the touched-table row they sit on.  Queued by the backward on its side stream - or, for
// calls with pfo_tgn_batch.seg_in_forward, by the forward on ITS side stream (beside layer 1, joined by the event layer 2 waits
// for anyway), which takes one event record and one wait off the backward's critical path.
static int seg_prologue(const Step& S, hipStream_t ss) {
  const Ws& w = S.w;
  // (deterministic: the table holds int64 fixed-point sums - rows of 2 D floats' worth)
  if (S.c->use_memory) RUN(pfo_zero_rows_launch(w.d_h0, w.n_core, S.capP, S.det ? 2 * S.d.D : S.d.D, S.n_rep, S.rep_stride, ss));
  RUN(pfo_seg_build_launch(w.idx0, w.nodes[0], (int)S.n[1], S.capP, S.b->uniform ? nullptr : w.cnt1, w.seg_ptr, w.seg_cur,
                           w.seg_tmp, w.seg_mem, w.seg_of, w.seg_scratch, ss));
  return PFO_OK;
}

// persist the lazily updated memory of the batch's positives + store their raw messages (tgn.py:290-317, 357-378)
static int state_update(const pfo_tgn_config* c, const pfo_tgn_state* st, const Ws& w, const int32_t* src, const int32_t* dst,
                        const double* ts, const int32_t* eidx, int32_t B, hipStream_t s) {
  pfo_tgn_layout lay;
  RUN(pfo_tgn_param_layout(c, &lay));
  const float* tw = st->params + lay.time_w;
  const float* tb = st->params + lay.time_b;
  // (the last-message-wins test needs the per-node table only for very large batches: memory.hip MSG_INLINE_MAX)
  int32_t* winner = pfo_msg_store_needs_winner(B) ? w.winner : nullptr;
  RUN(pfo_persist_launch(src, dst, B, w.slot, w.upd_mem, st->has_msg, st->msg_time, st->memory, st->last_update, c->D, winner, s));
  RUN(pfo_msg_store_launch(src, dst, ts, eidx, B, st->memory, st->last_update, st->edge_feat, tw, tb, c->D, c->Ef,
                           st->msg_table, st->msg_time, st->has_msg, winner, s));
  return PFO_OK;
}

// ---- the part of a forward call that depends on neither parameters nor gradients, in two halves (pfo_tgn_forward runs the
// GRU's weight-image launch between them; pfo_tgn_prepare runs them back to back on any stream, ahead of time)
static int prepare_sample(const Step& S, hipStream_t s) {
  const pfo_tgn_config* c = S.c; const pfo_tgn_state* st = S.st; const pfo_tgn_batch* b = S.b;
  const Ws& w = S.w; const int64_t* n = S.n;
  const int L = c->n_layers, K = b->K;
  void* stream = (void*)s;
  // The compaction's flags are cleared on THIS stream (4 us): a wait for a side-stream memset costs the waiting stream 5-17 us
  // on this part (r3 timeline), more than the memset itself.  Same reasoning for the GRU's two weight images below.
  // With two or more levels the UPPER level's sampler launch clears the flags (it does not mark) and the memset is gone
  // (fwd.begin -> fwd.sampled 40.4 -> 35.6 us).  Both levels of most-recent sampling in ONE launch (a workgroup per root: its
  // own query, then the 1 + K queries that depend on it) was built and measured too: it marks, so the memset comes back, and
  // the step does not move (1.302 / 1.308 against 1.297 / 1.305 ms, round 5) - removed again.
  // (only while the clear stays a small share of that launch: it runs on ceil(n * 16 / 256) workgroups, a memset on the
  //  whole chip - beyond ~4 K ints per workgroup (large node tables under small batches) the memset is the faster head)
  const int64_t clear_blocks = std::max<int64_t>(1, pfo_ceil_div(n[L] * 16, 256));
  const bool clear_in_sampler = L >= 2 && (w.mark_bytes % 4) == 0 && (int64_t)(w.mark_bytes / 4) <= 4096 * clear_blocks;
  if (!clear_in_sampler) HIPOK(hipMemsetAsync(w.mark, 0, w.mark_bytes, s), "memset failed");
  // ---- frontier expansion: K1 per level (utils.py:163-219 called from embedding_module.py:125).  Enqueued before the
  // side-stream work below: it depends on nothing else, and the GPU samples while the host is still enqueueing
  for (int l = L; l >= 1; --l) {
    const int64_t* dr = (b->uniform == 1) ? b->draws[L - l] : nullptr;
    PFO_REQUIRE(b->uniform != 1 || dr, "missing draws for a level");
    // level L reads the caller's roots directly; every level writes [its own nodes | their neighbours] as the next one
    const int32_t* lvl_nodes = (l == L) ? b->roots : w.nodes[l];
    const double* lvl_ts = (l == L) ? b->root_ts : w.ts[l];
    // the last launch writes the whole level-0 list [S_1 ; neighbours(S_1)]: it also sets the touched-node flags, so the
    // compaction needs no marking pass
    RUN(pfo_tnbr_sample_dev(st->indptr, st->adj_nbr, st->adj_eidx, st->adj_ts, c->n_nodes, lvl_nodes, lvl_ts, n[l], K,
                            b->uniform, dr, b->seed, b->offset + (uint64_t)l * 0x100000000ull, b->offset_dev, nullptr,
                            w.eidx[l], nullptr, w.dt[l], w.nodes[l - 1], l > 1 ? w.ts[l - 1] : nullptr, l == 1 ? w.mark : nullptr,
                            l == 1 ? w.cnt1 : nullptr, stream, (clear_in_sampler && l == L) ? w.mark : nullptr,
                            (clear_in_sampler && l == L) ? (int64_t)(w.mark_bytes / 4) : 0));
  }
  return PFO_OK;
}
static int prepare_compact(const Step& S, hipStream_t s) {
  const Ws& w = S.w;
  // slot[v] = row of v in the per-step tables (roots and every sampled neighbour, all levels; + the caller's extra nodes)
  return pfo_touch_compact_launch(nullptr, 0, S.b->extra_nodes, S.b->n_extra, S.c->n_nodes, w.mark, w.slot, w.touched, w.n_touched,
                                  w.scan, true, true, s);
}
static int prepare_pack(const Step& S, hipStream_t s) {
  const pfo_tgn_state* st = S.st;
  const Ws& w = S.w;
  const int D = S.d.D;
  // ---- level-0 rows of the touched nodes: memory' + node features (embedding_module.py:93-98), memory' = the lazily
  // updated memory (tgn.py:251; memory_updater.py:35-53).  One launch copies the rows the GRU reads (and the backward reads
  // again after the state update has overwritten the tables) and translates the level-0 list into table rows
  // (idx0[i] = row of the i-th level-0 reference).
  if (S.c->use_memory)
    return pfo_pack_remap_launch(st->msg_table, S.d.M, st->memory, D, st->has_msg, w.touched, w.n_touched, S.capP, w.msg_rows,
                                 w.h_rows, w.hm, w.nodes[0], S.n[0], w.slot, w.idx0, s);
  return pfo_pack_remap_launch(nullptr, S.d.M, st->node_feat, D, nullptr, w.touched, w.n_touched, S.capP, nullptr, w.h0_tab, nullptr,
                               w.nodes[0], S.n[0], w.slot, w.idx0, s);
}

// ---- Everything the step derives from the PARAMETERS alone, in two stages of small dependent launches on one stream
// (pfo_tgn_forward runs them on its side stream when the parameter cache is absent or stale; pfo_tgn_refresh right behind the
// optimizer).  Stage A: cos(b), the composite weights of every layer and the weight images layer 1 and the top layer's fc2
// need.  Stage B ("fc2 fold"): the composites of the layers >= 2 with the fc2 of the layer below folded in, and their images.
static int build_gru_images(const pfo_tgn_config* c, const Dims& d, const Ws& w, const Params& P, hipStream_t s, bool forward_only = false) {
  // gate-ordered rows: r | z | n_i | n_h per 16 hidden units (gemm_fused.hip gru_fused_kernel)
  const int D = d.D;
  PfoBimg im[2];
  im[0].src = P.w_ih; im[0].ld = d.Mg; im[0].N = 3 * D; im[0].K = d.Mg; im[0].trans = 0; im[0].dst = w.iWih;
  im[1].src = P.w_hh; im[1].ld = D; im[1].N = 3 * D; im[1].K = D; im[1].trans = 0; im[1].dst = w.iWhh;
  im[0].gate = 1; im[0].gate_D = D; im[1].gate = 2; im[1].gate_D = D;
  (void)c;
  RUN(pfo_bimg_launch(im, 2, s));
  if (d.Hm == 0) return PFO_OK;
  // the message MLP's operands, both ways: W1, W2 for the forward, W_ih^T and W2^T for d m = dgi W_ih, d hid = d m W2
  PfoBimg mm[4];
  auto img = [&](int i, const float* src, int64_t ld, int N_, int K_, int trans, void* dst) {
    mm[i].src = src; mm[i].ld = ld; mm[i].N = N_; mm[i].K = K_; mm[i].trans = trans; mm[i].dst = dst;
  };
  img(0, P.m_w1, d.M, d.Hm, d.M, 0, w.iMW1);
  img(1, P.m_w2, d.Hm, d.Mg, d.Hm, 0, w.iMW2);
  if (forward_only) return pfo_bimg_launch(mm, 2, s);             // (pfo_tgn_observe: no backward reads the transposed pair)
  img(2, P.w_ih, d.Mg, d.Mg, 3 * D, 1, w.iWihT);
  img(3, P.m_w2, d.Hm, d.Hm, d.Mg, 1, w.iMW2T);
  return pfo_bimg_launch(mm, 4, s);
}
// The MLP message function (modules/message_function.py:13-26) over the touched rows, in front of the lazy GRU:
// hid = relu(raw W1^T + b1), out = hid W2^T + b2.  raw rows: packed [rows, M] (idx null) or gathered from the message table.
// Rows without a pending message are computed like the others - the GRU keeps their memory row and their gate gradients are zero.
static int message_mlp(const Dims& d, const Params& P, const float* raw, const int32_t* idx, const void* iW1, const void* iW2,
                       float* hid, float* out, int cap_rows, const int32_t* n_rows, hipStream_t s) {
  PfoGemm g1 = g_nt(raw, d.M, idx, P.m_w1, d.M, hid, d.Hm, cap_rows, d.Hm, d.M, P.m_b1);
  g1.relu = 1; g1.m_dev = n_rows; g1.b_img = iW1;
  RUN(pfo_gemm_launch(g1, s));
  PfoGemm g2 = g_nt(hid, d.Hm, nullptr, P.m_w2, d.Hm, out, d.Mg, cap_rows, d.Mg, d.Hm, P.m_b2);
  g2.m_dev = n_rows; g2.b_img = iW2;
  return pfo_gemm_launch(g2, s);
}
static int build_stage_a(const Dims& d, const Ws& w, const Params& P, hipStream_t ss) {
  const int L = d.L, D = d.D, H = d.H, E = d.E, C = d.C, dh = d.dh, Cp = d.Cp, HCp = d.H * d.Cp;
  // 64 zero floats | Wqk / W1ovT / cqk of every layer: the builds below OVERWRITE the live rows and never touch the padding
  // rows / columns, which must be zero - in the workspace (recycled memory) that takes a memset per build, in the parameter
  // cache the caller cleared the buffer once when it allocated it (pfo_tgn_state.pcache: "zero-initialised")
  if (!w.pz_in_cache) HIPOK(hipMemsetAsync(w.pz, 0, w.pz_bytes, ss), "memset failed");
  RUN(pfo_time_encode(w.pz, 1, P.tw, P.tb, D, w.cosb, ss));                     // cos(fma(0, w, b)) (embedding_module.py:92)
  PfoGemm st1[3 * PFO_MAX_LAYERS], st2[4 * PFO_MAX_LAYERS];
  PfoBimg im[8 * PFO_MAX_LAYERS + 2];
  int n1 = 0, n2 = 0, ni = 0;
  auto img = [&](const float* src, int64_t ld, int N_, int K_, int trans, void* dst) {
    im[ni].src = src; im[ni].ld = ld; im[ni].N = N_; im[ni].K = K_; im[ni].trans = trans; im[ni].dst = dst; ++ni;
  };
  for (int l = 1; l <= L; ++l) {
    const LayerWs& lw = w.layer[l];
    const auto& p = P.l[l];
    PfoGemm* a1 = st1 + n1;
    a1[0] = g_nt(w.cosb, D, nullptr, p.wq + D, E, lw.cq, E, 1, E, D, p.b_in);            // cq = Wq[:, D:] cos(b) + bq
    a1[1] = g_nt(p.wo, E, nullptr, p.w1, E + D, lw.W1oT, D, E, D, E, nullptr);           // W1oT = Wo^T W1[:, :E]^T
    a1[1].a_kmajor = 1;
    a1[2] = g_nt(p.wk, C, nullptr, p.wq, E, lw.Wqk, D, C, D, dh, nullptr);               // Wqk_h = Wk_h^T Wq_h[:, :D]
    a1[2].a_kmajor = 1; a1[2].b_kmajor = 1; a1[2].batch = H;
    a1[2].a_bs[0] = (int64_t)dh * C; a1[2].b_bs[0] = (int64_t)dh * E; a1[2].c_bs = (int64_t)Cp * D;
    n1 += 3;
    PfoGemm* a2 = st2 + n2;
    a2[0] = g_nn(lw.cq, E, p.wk, C, lw.cqk, HCp, 1, C, dh);                               // cqk_h = Wk_h^T cq_h
    a2[0].batch = H; a2[0].a_bs[0] = dh; a2[0].b_bs[0] = (int64_t)dh * C; a2[0].c_bs = Cp;
    a2[1] = g_nt(p.wv, C, nullptr, lw.W1oT, D, lw.W1ovT, D, C, D, dh, nullptr);           // W1ovT_h = Wv_h^T W1oT_h
    a2[1].a_kmajor = 1; a2[1].b_kmajor = 1; a2[1].batch = H;
    a2[1].a_bs[0] = (int64_t)dh * C; a2[1].b_bs[0] = (int64_t)dh * D; a2[1].c_bs = (int64_t)Cp * D;
    a2[2] = g_nn(p.b_in + 2 * E, dh, lw.W1oT, D, lw.W1ovT + (int64_t)C * D, D, 1, D, dh); // row C: (W1 Wo_h bv_h)^T
    a2[2].batch = H; a2[2].a_bs[0] = dh; a2[2].b_bs[0] = (int64_t)dh * D; a2[2].c_bs = (int64_t)Cp * D;
    a2[3] = g_nt(p.bo, E, nullptr, p.w1, E + D, lw.W1ovT + (int64_t)(C + 1) * D, D, 1, D, E, nullptr);   // row C+1 of head 0: (W1 bo)^T
    n2 += 4;
    // fp16 images of this layer's weight operands, in both orientations (forward and data-gradient launches).
    // Layers >= 2 take theirs from the fc2-folded composites (stage B).
    if (l == 1) {
      // layer 1 projects the touched-node table once: [Wqk ; W1[:, E:]] stacked along the output dimension
      img(lw.Wqk, D, HCp, D, 0, w.iQX);        im[ni - 1].row0 = 0;   im[ni - 1].rows_total = HCp + D;
      img(p.w1 + E, E + D, D, D, 0, w.iQX);    im[ni - 1].row0 = HCp; im[ni - 1].rows_total = HCp + D; im[ni - 1].last = 1;
      img(lw.Wqk, D, D, HCp, 1, lw.iWqkT);
      img(lw.W1ovT, D, HCp, D, 0, lw.iW1ovT);  img(lw.W1ovT, D, D, HCp, 1, lw.iW1ov);
      img(p.w1 + E, E + D, D, D, 1, lw.iW1bT);
    }
    if (l == L) { img(p.w2, D, D, D, 0, lw.iW2); img(p.w2, D, D, D, 1, lw.iW2T); }   // only the top layer applies its fc2
  }
  for (int i = 0; i < n1; i += PFO_GEMM_MULTI_MAX) RUN(pfo_gemm_multi_launch(st1 + i, std::min(PFO_GEMM_MULTI_MAX, n1 - i), ss));
  for (int i = 0; i < n2; i += PFO_GEMM_MULTI_MAX) RUN(pfo_gemm_multi_launch(st2 + i, std::min(PFO_GEMM_MULTI_MAX, n2 - i), ss));
  for (int i = 0; i < ni; i += PFO_BIMG_MAX) RUN(pfo_bimg_launch(im + i, std::min(PFO_BIMG_MAX, ni - i), ss));
  return PFO_OK;
}
// fc2 fold.  A layer l >= 2 reads rows of the previous layer, out = A h + b (A = W2, b = b2 of layer l-1, h = that
// layer's h1 row).  Every use of such a row is linear, so A and b move into THIS layer's composites and the previous
// layer's fc2 contraction over all its instances (and, backward, d h1 = d out W2 and dW2 = d out^T h1) disappears:
//   query side   qk'_h = Q_h x + cqk_h,  x = A s + b        ->  T1_h = Q_h A,  t_h = Q_h b + cqk_h
//   scores       qk'_h,node . (A k + b) = (A^T qk'_h,node) . k + const(j)   (the constant drops out of the softmax)
//                                                         ->  Q_f,h = [A^T T1_h,node ; T1_h,edge|time],  c_f,h likewise from t_h
//   context      sum_j a'_j (A k_j + b) = A c + b sum_j a'_j  ->  V_f,h,node = A^T V_h,node,  V_f,h[C] = V_h[C] + b^T V_h,node
//   x term       W1b (A s + b)                              ->  W1b_f = W1b A,  b1_f = b1 + W1b b
// (Q_h = Wqk_h, V_h = W1ovT_h; tiny products, two more dependent stages.)
static int build_stage_b(const Dims& d, const Ws& w, const Params& P, hipStream_t ss) {
  const int L = d.L, D = d.D, H = d.H, E = d.E, C = d.C, Cp = d.Cp, HCp = d.H * d.Cp;
  if (L < 2) return PFO_OK;
  PfoGemm f1[4 * PFO_MAX_LAYERS], f2[4 * PFO_MAX_LAYERS];
  PfoBimg fim[6 * PFO_MAX_LAYERS];
  int m1 = 0, m2 = 0, mi = 0;
  const int64_t HCpD = (int64_t)HCp * D;
  for (int l = 2; l <= L; ++l) {
    const LayerWs& lw = w.layer[l];
    const auto& p = P.l[l];
    const float* A = P.l[l - 1].w2;
    const float* bv = P.l[l - 1].b2;
    PfoGemm* a = f1 + m1;
    a[0] = g_nn(lw.Wqk, D, A, D, lw.T1, D, HCp, D, D);                                    // T1 = Q A (all heads' rows)
    a[1] = g_nt(bv, D, nullptr, lw.Wqk, D, lw.tq, HCp, 1, HCp, D, lw.cqk);               // t = Q b + cqk
    a[2] = g_nn(p.w1 + E, E + D, A, D, lw.W1b_f, D, D, D, D);                            // W1b_f = W1b A
    a[3] = g_nt(bv, D, nullptr, p.w1 + E, E + D, lw.b1_f, D, 1, D, D, p.b1);             // b1_f = b1 + W1b b
    m1 += 4;
  }
  for (int i = 0; i < m1; i += PFO_GEMM_MULTI_MAX) RUN(pfo_gemm_multi_launch(f1 + i, std::min(PFO_GEMM_MULTI_MAX, m1 - i), ss));
  for (int l = 2; l <= L; ++l) {
    const LayerWs& lw = w.layer[l];
    const float* A = P.l[l - 1].w2;
    const float* bv = P.l[l - 1].b2;
    {
      // the rows the fold does not touch (edge | time, the two bias rows) come over as they are - ONE grouped launch instead of
      // three runtime blits (each a launch of its own in this chain of small dependent launches)
      PfoSumSlabs cp[3];
      cp[0].dst = lw.W1ovT_f; cp[0].src = lw.W1ovT; cp[0].count = HCpD;
      cp[1].dst = lw.Wqk_f;   cp[1].src = lw.T1;    cp[1].count = HCpD;
      cp[2].dst = lw.cqk_f;   cp[2].src = lw.tq;    cp[2].count = HCp;
      for (int q = 0; q < 3; ++q) { cp[q].n_slabs = 1; cp[q].accumulate = 0; cp[q].stride = 0; }
      RUN(pfo_sum_slabs_launch(cp, 3, ss));
    }
    PfoGemm* a = f2 + m2;
    a[0] = g_nn(A, D, lw.T1, D, lw.Wqk_f, D, D, D, D);        a[0].a_kmajor = 1;          // Q_f,node = A^T T1_node
    a[0].batch = H; a[0].b_bs[0] = (int64_t)Cp * D; a[0].c_bs = (int64_t)Cp * D;
    a[1] = g_nn(lw.tq, D, A, D, lw.cqk_f, D, 1, D, D);                                    // c_f,node = A^T t_node
    a[1].batch = H; a[1].a_bs[0] = Cp; a[1].c_bs = Cp;
    a[2] = g_nn(A, D, lw.W1ovT, D, lw.W1ovT_f, D, D, D, D);   a[2].a_kmajor = 1;          // V_f,node = A^T V_node
    a[2].batch = H; a[2].b_bs[0] = (int64_t)Cp * D; a[2].c_bs = (int64_t)Cp * D;
    a[3] = g_nn(bv, D, lw.W1ovT, D, lw.W1ovT_f + (int64_t)C * D, D, 1, D, D);             // V_f[C] = V[C] + b^T V_node
    a[3].batch = H; a[3].b_bs[0] = (int64_t)Cp * D; a[3].c_bs = (int64_t)Cp * D; a[3].accumulate = 1;
    m2 += 4;
    auto fimg = [&](const float* src, int64_t ld, int N_, int K_, int trans, void* dst) {
      fim[mi].src = src; fim[mi].ld = ld; fim[mi].N = N_; fim[mi].K = K_; fim[mi].trans = trans; fim[mi].dst = dst; ++mi;
    };
    fimg(lw.Wqk_f, D, HCp, D, 0, lw.iWqk);      fimg(lw.W1b_f, D, D, D, 0, lw.iW1b);
    fimg(lw.Wqk_f, D, D, HCp, 1, lw.iWqkT);     fimg(lw.W1b_f, D, D, D, 1, lw.iW1bT);
    fimg(lw.W1ovT_f, D, HCp, D, 0, lw.iW1ovT);  fimg(lw.W1ovT_f, D, D, HCp, 1, lw.iW1ov);
  }
  for (int i = 0; i < m2; i += PFO_GEMM_MULTI_MAX) RUN(pfo_gemm_multi_launch(f2 + i, std::min(PFO_GEMM_MULTI_MAX, m2 - i), ss));
  for (int i = 0; i < mi; i += PFO_BIMG_MAX) RUN(pfo_bimg_launch(fim + i, std::min(PFO_BIMG_MAX, mi - i), ss));
  return PFO_OK;
}

// =============================================================================================
extern "C" int64_t pfo_tgn_pcache_bytes(const pfo_tgn_config* c) {
  if (check_cfg(c) != PFO_OK) return -1;
  return carve(c, nullptr, nullptr, true).cache_bytes + 256;
}

extern "C" int pfo_tgn_refresh(const pfo_tgn_config* c, const pfo_tgn_state* st, void* stream) {
  if (int rc = check_cfg(c)) return rc;
  PFO_REQUIRE(st && st->params && st->pcache, "pfo_tgn_refresh needs parameters and a parameter cache");
  const Dims d = dims_of(c);
  const Ws w = carve(c, nullptr, st->pcache, true);       // (only the cache's buffers are used)
  pfo_tgn_layout lay;
  RUN(pfo_tgn_param_layout(c, &lay));
  Params P;
  bind(lay, st->params, P, d.L, c->use_memory != 0);
  Side& sd = side();
  PFO_REQUIRE(sd.ok, "could not create the side stream");
  hipStream_t s = (hipStream_t)stream, sr = sd.s2;
  PfoRange range("pfo_tgn_refresh");
  RUN(side_join(sd, s));
  // Forked from the caller's stream (behind the kernel that wrote the parameters, and behind every reader of the old
  // composites: the previous backward joined its side streams into that stream) onto the SECOND side stream, not joined.
  // The next forward's first side stream - which packs the touched rows as soon as the compaction is done - waits for pc_a
  // only in front of the event layer 1 waits for anyway, and for pc_b in front of the one layer 2 waits for: the caller's
  // stream itself never waits for this chain, and the row pack does not queue behind it (on one stream the ~15 dependent
  // launches of both stages sat in front of the pack: +45 us per step, measured).
  // (the GRU's two images stay on the caller's stream - one 4 us launch, as in the forward: the fused GRU launch reads them
  //  on that stream BEFORE the forward's wait for the side stream)
  if (c->use_memory) RUN(build_gru_images(c, d, w, P, s));
  HIPOK(hipEventRecord(sd.fork, s), "event record failed");
  HIPOK(hipStreamWaitEvent(sr, sd.fork, 0), "event wait failed");
  RUN(build_stage_a(d, w, P, sr));
  HIPOK(hipEventRecord(sd.pc_a, sr), "event record failed");
  RUN(build_stage_b(d, w, P, sr));
  HIPOK(hipEventRecord(sd.pc_b, sr), "event record failed");
  return PFO_OK;
}

// =============================================================================================
extern "C" int pfo_tgn_prepare(const pfo_tgn_config* c, const pfo_tgn_state* st, const pfo_tgn_batch* b, void* workspace,
                               void* stream) {
  if (int rc = check_cfg(c)) return rc;
  PFO_REQUIRE(st && workspace && b, "null argument");
  PFO_REQUIRE(st->indptr && st->adj_nbr && st->adj_eidx && st->adj_ts && st->node_feat, "null state");
  PFO_REQUIRE(!c->use_memory || (st->memory && st->msg_table && st->has_msg), "null memory state");
  Step S(side());
  RUN(open_step(S, c, st, b, workspace, stream));
  RUN(check_batch(c, b));
  PfoRange range("pfo_tgn_prepare");
  RUN(side_join(S.sd, S.s));
  RUN(prepare_sample(S, S.s));
  RUN(prepare_compact(S, S.s));
  return prepare_pack(S, S.s);
}

// =============================================================================================
// ---- the forward's side-stream work: composite weights of every layer and their fp16 images (build_stage_a / _b), the
// step's cleared accumulators, the row pack and the fused state update.  Enqueued after the sampling / compaction / GRU
// launches of the caller's stream (which need none of it): when the host is the slower side (small batches, profilers) the
// critical chain is already queued while these ~14 launches are being issued; layer 1 waits for them (forward_layer).  With a
// valid parameter cache (pfo_tgn_state.pcache_valid) NONE of the builds is launched: the side stream only clears the step's
// accumulators, packs the rows and runs the state update.
static int forward_side(const Step& S) {
  const pfo_tgn_state* st = S.st; const pfo_tgn_batch* b = S.b;
  const Ws& w = S.w; Side& sd = S.sd;
  hipStream_t ss = S.ss; const bool build = S.build;
  PFO_REQUIRE(hipMemsetAsync(w.zero, 0, w.zero_bytes, ss) == hipSuccess, "memset failed");   // w.zero, w.tickets, time-gradient bins
  // (a pfo_tgn_refresh chain may still be running on the second side stream: a rebuild waits for all of it, a call that uses
  //  the cache waits for its two stages where their results are first needed - no-ops when no refresh is outstanding)
  if (build && st->pcache && !S.capturing) HIPOK(hipStreamWaitEvent(ss, sd.pc_b, 0), "event wait failed");
  if (build) RUN(build_stage_a(S.d, w, S.P, ss));
  // (in front of the pack, not behind it: a cross-stream wait costs the waiting stream 5-17 us even when the event fired long
  //  ago, and the record below is what layer 1 waits for - stage A of a refresh is done ~80 us after the optimizer's kernel)
  if (!build && !S.capturing) HIPOK(hipStreamWaitEvent(ss, sd.pc_a, 0), "event wait failed");
  if (S.pack_side) {
    HIPOK(hipStreamWaitEvent(ss, sd.comp_done, 0), "event wait failed");
    RUN(prepare_pack(S, ss));
  }
  HIPOK(hipEventRecord(sd.layer[0], ss), "event record failed");      // layer 1 (and the top layer's fc2) can go
  if (S.d.L >= 2) {
    if (build) RUN(build_stage_b(S.d, w, S.P, ss));
    else if (!S.capturing) HIPOK(hipStreamWaitEvent(ss, sd.pc_b, 0), "event wait failed");
    if (S.fused_state) {
      // the batch's state update, here: behind the lazy GRU (whose rows it persists), beside layer 1, in front of the event
      // layer 2 waits for - persist + message store leave the critical path and are joined at no extra wait
      HIPOK(hipStreamWaitEvent(ss, sd.gru_done, 0), "event wait failed");
      RUN(state_update(S.c, st, w, b->upd_src, b->upd_dst, b->upd_ts, b->upd_eidx, b->upd_B, ss));
      if (b->seg_in_forward) RUN(seg_prologue(S, ss));       // (behind gru_done: the compaction and the row pack are done)
    }
    HIPOK(hipEventRecord(sd.fold_done, ss), "event record failed");
  }
  return PFO_OK;
}

// One attention layer = THREE large contractions around the neighbour-tile attention kernel (taken
// to its end).  With one query per instance every projection that touches only that instance folds into a
// per-step composite weight:
//   qk'_h  = Wqk_h x + cqk_h,            Wqk_h  = Wk_h^T Wq_h[:, :D],   cqk_h = Wk_h^T (Wq_h[:, D:] cos(b) + bq_h)
//   h1     = relu( sum_h W1ov_h ctx'_h + W1[:, E:] x + b1 ),
//            W1ov_h = W1[:, :E] Wo[:, h] Wv_h   (fc1 . out_proj . value projection),
//            ctx'_h = [ sum_j a'_jh key_j | sum_j a'_jh | valid ]  - the two extra columns carry the folded value
//            bias (W1 Wo_h bv_h, scaled by the post-dropout weight sum) and the folded out_proj bias (W1 bo, only
//            on rows that have a valid neighbour: temporal_attention.py:84 zero-fills the others)
//   out    = W2 h1 + b2
// 0.60 MFLOP per instance instead of 1.13 (and 10.3 un-folded); Q, O and attn_out are never formed.
static int forward_layer(const Step& S, int l, float* emb_out) {
  PfoRange range_layer(LAYER_NAMES[NM_FWD][l]);
  const Ws& w = S.w;
  Side& sd = S.sd;
  hipStream_t s = S.s;
  const int D = S.d.D, HCp = S.d.H * S.d.Cp, WQ = HCp + D;
  const LayerView v = layer_view(S, l);   // layers >= 2 read the previous layer's h1 rows: its fc2 lives in this layer's folded composites
  const LayerWs& lw = *v.lw;
  const auto& p = S.P.l[l];
  const int N = v.N;
  if (l == 1) HIPOK(hipStreamWaitEvent(s, sd.layer[0], 0), "event wait failed");   // composite weights and layer 1's images are ready
  // ... and the fc2-folded ones of the layers >= 2.  (Round 3 tried ONE wait for both, on the later event: the side stream's
  // chain - 14 small dependent launches, ~150 us - then ends about when this stream reaches layer 1, and the touched-table
  // projection started 25 us late; layer 1 needs only the first ~90 us of that chain.)
  if (l == 2) HIPOK(hipStreamWaitEvent(s, sd.fold_done, 0), "event wait failed");
  // ---- qk' = x Wqk^T + cqk.  Layer 1: x is a row of the touched-node table, shared by every instance that sits on
  // that node (~54 k instances on ~11 k nodes at C2): ONE projection of the table, [qk' | x W1[:, E:]^T] per row
  if (l == 1) {
    PfoGemm g = g_nt(w.h0_tab, D, nullptr, lw.Wqk, D, w.QX, WQ, S.capP, WQ, D, w.l1_bias);
    g.m_dev = w.n_core; g.b_img = w.iQX;                 // (rows only the caller's extra list names are never queried)
    RUN(pfo_gemm_launch(g, s));
  } else {
    PfoGemm g = g_nt(v.xA, D, v.x_idx, v.Wqk, D, lw.QK, HCp, N, HCp, D, v.cqk);
    g.b_img = lw.iWqk;
    RUN(pfo_gemm_launch(g, s));
  }
  const PfoAttn a = attn_of(S, v);
  PFO_MARK(LAYER_NAMES[NM_QK][l], s);
  RUN(pfo_attn_fwd_launch(a, s));
  PFO_MARK(LAYER_NAMES[NM_AT][l], s);
  // ---- h1 = relu(ctx' W1ovT + x W1[:, E:]^T + b1)   (MergeLayer fc1 with out_proj and the value projection folded in)
  if (l == 1) {
    // the x term was projected with the table: it arrives as a row-gathered addend of the epilogue
    PfoGemm g = g_nn(lw.ctx, HCp, lw.W1ovT, D, lw.h1, D, N, D, HCp);
    g.bias = p.b1; g.relu = 1; g.b_img = lw.iW1ov;
    g.add_src = w.QX + HCp; g.add_ld = WQ; g.add_idx = w.idx0;
    RUN(pfo_gemm_launch(g, s));
  } else {
    // both K-concatenated sources ([ctx' | x] against [W1ov | W1[:, E:]]) in one launch: h1 is written once
    PfoGemm g = g_nn(lw.ctx, HCp, v.W1ovT, D, lw.h1, D, N, D, HCp);
    g.A[1] = v.xA; g.lda[1] = D; g.a_idx[1] = v.x_idx; g.B[1] = v.W1b; g.ldb[1] = v.W1b_ld; g.K[1] = D;
    g.bias = v.b1; g.relu = 1; g.b_img = lw.iW1ov; g.b_img2 = lw.iW1b;
    RUN(pfo_gemm_launch(g, s));
  }
  PFO_MARK(LAYER_NAMES[NM_H1][l], s);
  if (l == S.d.L) {
    // out = W2 h1 + b2: only the top layer's rows ARE embeddings (N == R; written in place, no copy) - below it the
    // contraction is folded into the next layer's composites
    PfoGemm g = g_nt(lw.h1, D, nullptr, p.w2, D, emb_out, D, N, D, D, p.b2);
    g.b_img = lw.iW2;
    RUN(pfo_gemm_launch(g, s));
  }
  return PFO_OK;
}

extern "C" int pfo_tgn_forward(const pfo_tgn_config* c, const pfo_tgn_state* st, const pfo_tgn_batch* b, void* workspace,
                               float* emb_out, void* stream) {
  if (int rc = check_cfg(c)) return rc;
  PFO_REQUIRE(st && workspace && emb_out, "null argument");
  PFO_REQUIRE(st->indptr && st->adj_nbr && st->adj_eidx && st->adj_ts && st->node_feat && st->params, "null state");
  PFO_REQUIRE(c->Ef == 0 || st->edge_feat, "null edge features");
  PFO_REQUIRE(!c->use_memory || (st->memory && st->last_update && st->msg_table && st->msg_time && st->has_msg),
              "null memory state");
  Step S(side());
  RUN(open_step(S, c, st, b, workspace, stream));
  RUN(check_batch(c, b));
  S.build = !st->pcache || !st->pcache_valid;            // composites / images (re)built by this call
  S.fused_state = b->upd_src != nullptr && c->use_memory && S.d.L >= 2;
  PFO_REQUIRE(!S.fused_state || (b->upd_dst && b->upd_ts && b->upd_eidx && b->upd_B >= 1), "bad state-update arguments");
  const Ws& w = S.w; Side& sd = S.sd;
  hipStream_t s = S.s, ss = S.ss;

  PfoRange range_call(b->training ? "pfo_tgn_forward (training)" : "pfo_tgn_forward");
  PFO_REQUIRE(sd.ok, "could not create the side stream");
  // Everything on the side stream depends on the parameters only, so it may start at once (after whatever the main
  // stream did before this call); all layers share each launch.
  const bool bind_events = !S.capturing;                 // events bound to a launch (common.hpp): not under capture
  PFO_MARK("fwd.begin", s);
  // (with a deferred backward end in flight the side stream already waits for the caller's stream's last launch of that
  //  backward, and everything this call gives it either reads parameters only or sits behind an event of this call: no fork)
  // (only for the stream that queued the deferred backward: the side stream waits for THAT stream's last launch; a writer of
  //  the parameters on any other stream - a native optimizer step there, a graph replay - is ordered by the fork below)
  if (!(sd.pending_for(s) && sd.deferred_from == s && bind_events)) {
    HIPOK(hipEventRecord(sd.fork, s), "event record failed");
    HIPOK(hipStreamWaitEvent(ss, sd.fork, 0), "event wait failed");
  }
  if (!b->prepared) RUN(prepare_sample(S, s));
  PFO_MARK("fwd.sampled", s);
  // a deferred backward end + optimizer step of the previous step may still be running on the side stream: the sampling above
  // reads neither its buffers nor the parameters; everything below does (compaction counts, the GRU's weights ...)
  // (early: needs the fused state update's ordering - persist / message store run on the side stream behind every bucket -
  //  and layers >= 2 wait for fold_done, recorded there too; the top layer's raw b2 is the only late-bucket value this stream reads)
  RUN(side_join(sd, s, c->n_layers >= 2));
  PFO_MARK("fwd.side_joined", s);

  // the GRU contractions come first on the main stream: their two weight images are made there too (one 4 us launch)
  if (c->use_memory && S.build) RUN(build_gru_images(c, S.d, w, S.P, s));

  // ---- the nodes this step reads, compacted, and their level-0 rows packed (prepare_compact, prepare_pack; a prepared batch has them)
  // With memory the row pack leaves the caller's stream: the fused GRU gathers its rows straight from the per-node tables, and
  // the packed copies (for the backward, which runs after the state update has overwritten the tables) + the level-0 remap
  // (first used by layer 1's attention) are made on the side stream, in front of the event layer 1 waits for anyway.
  S.pack_side = c->use_memory && !b->prepared;
  if (S.pack_side) {
    // (comp_done rides on the completion of the compaction's LAST launch - its only one, or the third when the caller's extra
    //  list is marked and compacted too (data-parallel ranks: memory.hip pfo_touch_compact_launch): no marker packet)
    PFO_RUN_BOUND(bind_events, sd.comp_done, b->n_extra > 0 ? 2 : 0, s, prepare_compact(S, s));
    if (!bind_events) HIPOK(hipEventRecord(sd.comp_done, s), "event record failed");
  } else if (!b->prepared) {
    RUN(prepare_compact(S, s));
    RUN(prepare_pack(S, s));
  }
  PFO_MARK("fwd.compacted", s);
  if (c->use_memory) {
    PfoRange range_gru("forward lazy GRU");
    // both GRU contractions and the gate math in ONE launch (gemm_fused.hip gru_fused_kernel): gi / gh never exist in HBM
    const bool mlp = S.d.Hm > 0;
    if (mlp) {
      RUN(message_mlp(S.d, S.P, S.pack_side ? st->msg_table : w.msg_rows, S.pack_side ? w.touched : nullptr, w.iMW1, w.iMW2,
                      w.mlp_hid, w.mlp_out, S.capP, w.n_touched, s));
      PFO_MARK("fwd.msg_mlp", s);
    }
    PfoGruFused f;
    f.msg_rows = mlp ? w.mlp_out : w.msg_rows; f.K_msg = S.d.Mg; f.h_rows = w.h_rows; f.img_ih = w.iWih; f.img_hh = w.iWhh;
    f.b_ih = S.P.b_ih; f.b_hh = S.P.b_hh; f.hm = w.hm; f.touched = w.touched; f.node_feat = st->node_feat;
    f.upd_mem = w.upd_mem; f.h0_tab = w.h0_tab; f.gates = w.gates; f.D = S.d.D; f.cap_rows = S.capP; f.n_rows = w.n_touched;
    if (S.pack_side) { f.gather = mlp ? 2 : 1; if (!mlp) f.msg_rows = st->msg_table; f.h_rows = st->memory; f.hm = st->has_msg; }
    PFO_RUN_BOUND(S.fused_state && bind_events, sd.gru_done, 0, s, pfo_gru_fused_launch(f, s));
    if (S.fused_state && !bind_events) HIPOK(hipEventRecord(sd.gru_done, s), "event record failed");
    PFO_MARK("fwd.gru", s);
  }
  RUN(forward_side(S));
  for (int l = 1; l <= S.d.L; ++l) RUN(forward_layer(S, l, emb_out));
  PFO_MARK("fwd.end", s);
  return PFO_OK;
}

// =============================================================================================
extern "C" int pfo_tgn_grad_split(const pfo_tgn_config* c, int64_t* split) {
  if (int rc = check_cfg(c)) return rc;
  PFO_REQUIRE(split != nullptr, "null output");
  pfo_tgn_layout lay;
  RUN(pfo_tgn_param_layout(c, &lay));
  *split = c->n_layers >= 2 ? lay.layer[c->n_layers - 1].wq : lay.total;
  return PFO_OK;
}

// ---- The backward, stage by stage; pfo_tgn_backward_ev calls the stages in issue order.  Per layer: data gradients first (a
// chain of GEMMs + the attention core); every weight / bias gradient of the layer is then taken in ONE grouped split-K launch
// (bias gradients ride along as an extra column).
namespace {
// A layer's chain back to the parameters (unfold_fc2, chain_composites), issued by the host one layer later (pfo_tgn_backward_ev)
struct Chain { int l = 0; PfoTnProblem tn[4]; int ntn = 0; };
struct LayerBack {                 // what the stages of one layer hand to each other
  LayerView v;
  const float* dh1 = nullptr;      // d loss / d (fc1 pre-activation)
  Chain ch;                        // the layer's weight gradients over the instances, for its chain
  int n_tn_a = 0;                  // (the first n_tn_a of them need only d out, h1, ctx' and dh1)
  int dqk_by_member = 0;           // the attention backward took the run-merged kernel: dQK row m belongs to the m-th member
};
}  // namespace

static PfoTnProblem tn_of(const float* A, int64_t lda, const float* B, int64_t ldb, const int32_t* b_idx, int M_, int N_, float* C_,
                          int64_t ldc, float* bias_out) {
  PfoTnProblem q;
  q.A = A; q.lda = lda; q.B = B; q.ldb = ldb; q.b_idx = b_idx; q.M = M_; q.N = N_; q.C = C_; q.ldc = ldc; q.bias_out = bias_out;
  return q;
}
static int side_mean_once(Step& S) {
  const float* src = S.mean_src;
  S.mean_src = nullptr;
  return src ? pfo_mean_launch(src, S.mean_n, S.mean_out, S.ss) : PFO_OK;
}

// Stage 1, the side stream's opening work: the loss mean the caller left to this call, the cleared level-0 gradient rows and
// the layer-1 instance groups (seg_prologue: needed only when the layer-1 gradients are summed per row, late in this call -
// built beside the layer-L .. 2 work; layer 1's attention backward waits for seg_done).  A call whose forward already queued
// the last two (pfo_tgn_batch.seg_in_forward) forks nothing here - an event record costs the caller's stream a ~6 us bubble in
// front of its next kernel - and takes the mean behind the first event the side stream waits for anyway.
static int backward_open(Step& S) {
  if (S.seg_fwd) return PFO_OK;
  HIPOK(hipEventRecord(S.sd.fork, S.s), "event record failed");
  HIPOK(hipStreamWaitEvent(S.ss, S.sd.fork, 0), "event wait failed");
  RUN(side_mean_once(S));
  RUN(seg_prologue(S, S.ss));
  HIPOK(hipEventRecord(S.sd.seg_done, S.ss), "event record failed");
  return PFO_OK;
}

// Stage 2, top layer only: it applies its fc2 (utils.py:17): dW2 / db2 and d h1 = relu'(.) (d out W2).  (Below the top the
// layer above wrote d h1 directly, ReLU mask applied by its producers - attention backward's key rows, the x-side
// contraction's epilogue: fc2 is part of that layer's composites.)
static int backward_top_dh1(const Step& S, LayerBack& lb) {
  const int D = S.d.D, l = lb.v.l;
  const LayerWs& lw = *lb.v.lw;
  lb.ch.tn[lb.ch.ntn++] = tn_of(S.d_emb, D, lw.h1, D, nullptr, D, D, S.G.l[l].w2, D, S.G.l[l].b2);
  PfoGemm q = g_nn(S.d_emb, D, S.P.l[l].w2, D, S.w.dh1, D, lb.v.N, D, D);
  q.relu_src = lw.h1; q.relu_ld = D;                     // ReLU backward
  q.b_img = lw.iW2T;
  RUN(pfo_gemm_launch(q, S.s));
  PFO_MARK(LAYER_NAMES[NM_DH1][l], S.s);
  lb.dh1 = S.w.dh1;
  return PFO_OK;
}

// Stage 3: merged fc1, d ctx' = dh1 W1ovT^T (dx = dh1 W1[:, E:] is taken together with the query/key part, stage 5), and at
// layer 1 the weight gradients over the INSTANCES (dW2 / db2 at the top, dW1ovT).  Those need only d out, h1, ctx' and dh1: they
// go to the side stream.  With the bf16x3 tile they were best started as soon as dh1 existed, beside the d ctx' contraction
// (15 us/step better than next to the attention backward alone, whose single-wavefront workgroups starved a 74 KB-LDS kernel of
// slots); the fp16 tile (49 KB, half the matrix work) does better behind d ctx', beside the attention backward: 1.4495 against
// 1.4532 ms over four interleaved pairs.  (Behind the attention backward, beside the serial tail: +2 % per step.)
static int backward_dctx(Step& S, LayerBack& lb) {
  const Ws& w = S.w; Side& sd = S.sd; const pfo_tgn_batch* b = S.b;
  hipStream_t s = S.s, ss = S.ss;
  const LayerView& v = lb.v;
  const int l = v.l, N = v.N, D = S.d.D, HCp = S.d.H * S.d.Cp;
  const bool bind_events = !S.capturing;
  lb.ch.tn[lb.ch.ntn] = tn_of(v.lw->ctx, HCp, lb.dh1, D, nullptr, HCp, D, v.dW1ovT, D, nullptr);       // dW1ovT = ctx'^T dh1
  lb.ch.tn[lb.ch.ntn++].c_accumulate = 0;
  lb.n_tn_a = lb.ch.ntn;
  PfoGemm q = g_nt(lb.dh1, D, nullptr, v.W1ovT, D, w.dctx, HCp, N, HCp, D, nullptr);
  q.b_img = v.lw->iW1ovT;
  const bool bind_tn_a = bind_events && l == 1 && !pfo_prof_on();
  PFO_RUN_BOUND(bind_tn_a, sd.tn_a, 0, s, pfo_gemm_launch(q, s));
  PFO_MARK(LAYER_NAMES[NM_DCTX][l], s);
  if (l == 1 && b->mid_event && !b->mid_event_late) HIPOK(hipEventRecord((hipEvent_t)b->mid_event, s), "event record failed");
  if (l > 1) {
    lb.ch.tn[lb.ch.ntn] = tn_of(lb.dh1, D, v.xA, D, v.x_idx, D, D, v.lw->dW1b_f, D, v.lw->db1_f);      // d (W1[:, E:] A), d (b1 + W1[:, E:] b)
    lb.ch.tn[lb.ch.ntn].c_accumulate = 0; lb.ch.tn[lb.ch.ntn++].bias_accumulate = 0;
    return PFO_OK;
  }
  if (pfo_prof_on()) {        // event-bracketed step (bench.py's roofline sample): serial, so the bracket times the kernel alone
    RUN(pfo_gemm_tn_group_launch(lb.ch.tn, lb.n_tn_a, N, nullptr, w.slabs, w.slab_floats, s));
    HIPOK(hipEventRecord(sd.tn_a_done, s), "event record failed");
    return PFO_OK;
  }
  if (!bind_events) HIPOK(hipEventRecord(sd.tn_a, s), "event record failed");     // (bound: tn_a rides on the d ctx' launch)
  HIPOK(hipStreamWaitEvent(ss, sd.tn_a, 0), "event wait failed");
  RUN(side_mean_once(S));
  PFO_MARK("@side1.tn_a.begin", ss);
  RUN(pfo_gemm_tn_group_launch(lb.ch.tn, lb.n_tn_a, N, nullptr, w.slabs2, w.slab_floats, ss));
  PFO_MARK("@side1.tn_a.end", ss);
  HIPOK(hipEventRecord(sd.tn_a_done, ss), "event record failed");
  return PFO_OK;
}

// Stage 4: the attention core
static int backward_attn(Step& S, LayerBack& lb) {
  const Ws& w = S.w; const pfo_tgn_config* c = S.c; const pfo_tgn_batch* b = S.b;
  hipStream_t s = S.s;
  const LayerView& v = lb.v;
  const int l = v.l, D = S.d.D;
  PfoAttn a = attn_of(S, v);
  a.nbr_relu = v.folded ? 1 : 0;                               // the keys are h1 rows of the layer below: d row *= (row > 0)
  a.dctx = w.dctx; a.dQK = v.dqk;
  if (l == 1) { a.d_nbr = c->use_memory ? w.d_h0 : nullptr; a.d_nbr_ld = D; a.d_nbr_rep = S.rep_stride; a.d_nbr_nrep = S.n_rep; }
  else        { a.d_nbr = w.dH[l - 1]; a.d_nbr_ld = D; }
  a.dtime_part = w.dtime;
  a.det = S.det; a.dtime_slab = w.dtime_slab + S.det_rows * 2 * D;
  int n_parts = 0;
  if (l == 1 && c->use_memory && !S.seg_fwd) HIPOK(hipStreamWaitEvent(s, S.sd.seg_done, 0), "event wait failed");   // d_h0 is clear, the groups exist
  if (l == 1 && c->use_memory && !b->uniform) {
    // key-side gradients of instances with identical neighbour lists leave as one set of atomics (attn_bwd_runs.hip)
    a.members = w.seg_mem; a.seg_ptr = w.seg_ptr; a.n_rows = w.n_core; a.run_cnt = w.cnt1; a.dqk_live = w.dqk_live;
  }
  lb.dqk_by_member = pfo_attn_bwd_uses_runs(a) ? 1 : 0;
  RUN(pfo_attn_bwd_launch(a, &n_parts, s));
  PFO_MARK(LAYER_NAMES[NM_BATTN][l], s);
  if (l == 1 && b->mid_event && b->mid_event_late) HIPOK(hipEventRecord((hipEvent_t)b->mid_event, s), "event record failed");
  if (S.det) S.det_rows += n_parts;
  return PFO_OK;
}

// Stage 5, layer 1 - merged query/key projection: dx += dqk' Wqk, dWqk = dqk'^T x, gqk = colsum(dqk').  x is a row of the
// touched-node table shared by all instances on that node, so everything that is linear in the per-instance gradients (dqk',
// dh1) and otherwise depends on x only - the data gradient of x and the two weight gradients against x - is taken AFTER summing
// those gradients per table row: contractions over the ~11 k touched rows instead of the ~54 k instances.
static int backward_table_side(Step& S, const LayerBack& lb) {
  const Ws& w = S.w; Side& sd = S.sd;
  hipStream_t s = S.s, ss = S.ss;
  const LayerWs& lw = *lb.v.lw;
  const auto& p = S.P.l[1]; const auto& g = S.G.l[1];
  const int D = S.d.D, E = S.d.E, HCp = S.d.H * S.d.Cp, WQ = HCp + D, capP = S.capP;
  const bool bind_events = !S.capturing;
  if (!S.c->use_memory) HIPOK(hipStreamWaitEvent(s, sd.seg_done, 0), "event wait failed");   // (with memory: awaited before the attention backward)
  PFO_RUN_BOUND(bind_events, sd.tn_b, 0, s,
                pfo_segsum_launch(lb.v.dqk, HCp, lb.dh1, D, w.seg_ptr, w.seg_mem, w.seg_of, S.n[1], w.n_core, capP, lb.dqk_by_member,
                                  lb.dqk_by_member ? w.dqk_live : nullptr, w.Dq, s));   // Dq = [sum dqk' | sum dh1]
  // the weight gradients over the table rows go to the side stream too (beside d h0 / the GRU backward on this one)
  if (!bind_events) HIPOK(hipEventRecord(sd.tn_b, s), "event record failed");
  PFO_MARK("bwd.L1.segsum", s);
  HIPOK(hipStreamWaitEvent(ss, sd.tn_b, 0), "event wait failed");
  RUN(side_mean_once(S));
  PfoTnProblem tb[2];
  tb[0] = tn_of(w.Dq, WQ, w.h0_tab, D, nullptr, HCp, D, lw.dWqk, D, lw.gqk);               // dWqk = (sum dqk')^T h0, gqk
  tb[0].c_accumulate = 0; tb[0].bias_accumulate = 0;
  tb[1] = tn_of(w.Dq + HCp, WQ, w.h0_tab, D, nullptr, D, D, g.w1 + E, E + D, g.b1);        // dW1[:, E:], db1
  // (the layer's chain-back on the side stream needs dWqk / gqk: this launch stays there also while profiling)
  PFO_MARK("@side1.tn_b.begin", ss);
  RUN(pfo_gemm_tn_group_launch(tb, 2, capP, w.n_core, w.slabs2, w.slab_floats, ss));
  PFO_MARK("@side1.tn_b.end", ss);
  if (S.c->use_memory) {
    // d h0_tab (query side) = Dq [Wqk ; W1[:, E:]]; the GRU backward adds it to the key-side rows the attention scattered
    PfoGemm q = g_nn(w.Dq, WQ, lw.Wqk, D, w.dx_tab, D, capP, D, HCp);
    q.A[1] = w.Dq + HCp; q.lda[1] = WQ; q.B[1] = p.w1 + E; q.ldb[1] = E + D; q.K[1] = D;
    q.b_img = lw.iWqkT; q.b_img2 = lw.iW1bT; q.m_dev = w.n_core;
    RUN(pfo_gemm_launch(q, s));
    PFO_MARK(LAYER_NAMES[NM_DX][1], s);
  }
  return PFO_OK;
}
// Stage 5, layers >= 2 - d h1 of the layer below, self rows [0, N): [dqk' | dh1] [Q_f ; W1b_f], masked by that layer's ReLU.
// Both sources in one launch, dx written once.  The launch carries (or is followed by the record of) layer[l], the event that
// releases the layer's chain on the device.
static int backward_x_side(const Step& S, LayerBack& lb) {
  const LayerView& v = lb.v;
  const int l = v.l, D = S.d.D, HCp = S.d.H * S.d.Cp;
  const bool bind_events = !S.capturing;
  PfoGemm q = g_nn(v.dqk, HCp, v.Wqk, D, v.dx, D, v.N, D, HCp);
  q.A[1] = lb.dh1; q.lda[1] = D; q.B[1] = v.W1b; q.ldb[1] = v.W1b_ld; q.K[1] = D;
  q.b_img = v.lw->iWqkT; q.b_img2 = v.lw->iW1bT;
  q.relu_src = v.xA; q.relu_ld = D;
  PFO_RUN_BOUND(bind_events, S.sd.layer[l], 0, S.s, pfo_gemm_launch(q, S.s));
  PFO_MARK(LAYER_NAMES[NM_DX][l], S.s);
  lb.ch.tn[lb.ch.ntn] = tn_of(v.dqk, HCp, v.xA, D, v.x_idx, HCp, D, v.dWqk, D, v.gqk);
  lb.ch.tn[lb.ch.ntn].c_accumulate = 0; lb.ch.tn[lb.ch.ntn++].bias_accumulate = 0;
  // (launched by unfold_fc2, on the second side stream in front of the layer's chain: nothing on this stream needs the weight
  //  gradients of a layer >= 2 - 36 us of launch-latency-bound work off the critical path at C2)
  if (!bind_events) HIPOK(hipEventRecord(S.sd.layer[l], S.s), "event record failed");
  return PFO_OK;
}

// Stage 6, layers >= 2: their weight gradients, then the fc2 fold undone (notation of build_stage_b: A, b = W2, b2 of layer
// l-1; Q = Wqk, V = W1ovT, per head):
//   dT1_node = A dQ_f,node      dT1_edge|time = dQ_f,edge|time         dt likewise from gqk_f
//   dV_node  = A dV_f,node + b (x) dV_f[C]         dV elsewhere = dV_f
//   dW1b     = dW1b_f A^T + db1_f (x) b            db1 += db1_f
//   dQ       = dT1 A^T + dt (x) b                  d cqk = dt
//   dA       = sum_h ( T1_node dQ_f,node^T + t_node (x) gqk_f,node + V_node dV_f,node^T ) + W1b^T dW1b_f + Q^T dT1
//   db       = sum_h V_node dV_f[C]^T + W1b^T db1_f + Q^T dt
// The dA / db terms are written to slabs (several heads add to one matrix) and summed once.
static int unfold_fc2(const Step& S, const Chain& ch) {
  const Ws& w = S.w; Side& sd = S.sd;
  const int l = ch.l, N = (int)S.n[l];
  const LayerWs& lw = w.layer[l];
  const auto& p = S.P.l[l];
  const auto &g = S.G.l[l], &gp = S.G.l[l - 1];
  const int D = S.d.D, H = S.d.H, E = S.d.E, C = S.d.C, Cp = S.d.Cp, HCp = H * Cp;
  const float *A = S.P.l[l - 1].w2, *bv = S.P.l[l - 1].b2;
  const int64_t HCpD = (int64_t)HCp * D, CpD = (int64_t)Cp * D, DD = (int64_t)D * D;
  // (on the second side stream: the first one must stay free for layer 1's weight gradients over the instances)
  hipStream_t sf = S.s2;
  HIPOK(hipStreamWaitEvent(sf, sd.layer[l], 0), "event wait failed");
  if (pfo_prof_on()) {
    // event-bracketed step (bench.py's roofline sample): on the caller's stream, so that the bracket times the kernel alone
    RUN(pfo_gemm_tn_group_launch(ch.tn, ch.ntn, N, nullptr, w.slabs, w.slab_floats, S.s));
    HIPOK(hipEventRecord(sd.layer[l], S.s), "event record failed");
    HIPOK(hipStreamWaitEvent(sf, sd.layer[l], 0), "event wait failed");
  } else {
    RUN(pfo_gemm_tn_group_launch(ch.tn, ch.ntn, N, nullptr, w.slabs3, w.slab_floats, sf));
  }
  {
    PfoSumSlabs cp[3];                        // (one grouped launch instead of three runtime blits, as in build_stage_b)
    cp[0].dst = lw.dT1;    cp[0].src = lw.dWqk_f;   cp[0].count = HCpD;
    cp[1].dst = lw.gqk;    cp[1].src = lw.gqk_f;    cp[1].count = HCp;
    cp[2].dst = lw.dW1ovT; cp[2].src = lw.dW1ovT_f; cp[2].count = HCpD;
    for (int q = 0; q < 3; ++q) { cp[q].n_slabs = 1; cp[q].accumulate = 0; cp[q].stride = 0; }
    RUN(pfo_sum_slabs_launch(cp, 3, sf));
  }
  float* sl = lw.fold_slabs;
  float* vs = lw.fold_vslabs;
  {
    PfoGemm u[9];
    u[0] = g_nn(A, D, lw.dWqk_f, D, lw.dT1, D, D, D, D);                                  // dT1_node = A dQ_f,node
    u[0].batch = H; u[0].b_bs[0] = CpD; u[0].c_bs = CpD;
    u[1] = g_nt(lw.gqk_f, D, nullptr, A, D, lw.gqk, D, 1, D, D, nullptr);                 // dt_node = A gqk_f,node
    u[1].batch = H; u[1].a_bs[0] = Cp; u[1].c_bs = Cp;
    u[2] = g_nt(lw.T1, D, nullptr, lw.dWqk_f, D, sl, D, D, D, D, nullptr);                // slab h: T1_node dQ_f,node^T
    u[2].batch = H; u[2].a_bs[0] = CpD; u[2].b_bs[0] = CpD; u[2].c_bs = DD;
    u[3] = g_nt(lw.W1ovT, D, nullptr, lw.dW1ovT_f, D, sl + H * DD, D, D, D, D, nullptr);  // slab H+h: V_node dV_f,node^T
    u[3].batch = H; u[3].a_bs[0] = CpD; u[3].b_bs[0] = CpD; u[3].c_bs = DD;
    u[4] = g_nn(p.w1 + E, E + D, lw.dW1b_f, D, sl + 2 * H * DD, D, D, D, D);              // slab 2H: W1b^T dW1b_f
    u[4].a_kmajor = 1;
    u[5] = g_nn(A, D, lw.dW1ovT_f, D, lw.dW1ovT, D, D, D, D);                             // dV_node = A dV_f,node
    u[5].batch = H; u[5].b_bs[0] = CpD; u[5].c_bs = CpD;
    u[6] = g_nt(lw.dW1ovT_f + (int64_t)C * D, D, nullptr, lw.W1ovT, D, vs, D, 1, D, D, nullptr);   // vslab h: V_node dV_f[C]^T
    u[6].batch = H; u[6].a_bs[0] = CpD; u[6].b_bs[0] = CpD; u[6].c_bs = D;
    u[7] = g_nn(lw.db1_f, D, p.w1 + E, E + D, vs + H * D, D, 1, D, D);                    // vslab H: W1b^T db1_f
    u[8] = g_nt(lw.dW1b_f, D, nullptr, A, D, g.w1 + E, E + D, D, D, D, nullptr);          // dW1[:, E:] += dW1b_f A^T
    u[8].accumulate = 1;
    RUN(pfo_gemm_multi_launch(u, 9, sf));
  }
  {
    PfoGemm u[3];
    u[0] = g_nt(lw.dT1, D, nullptr, A, D, lw.dWqk, D, HCp, D, D, nullptr);                // dQ = dT1 A^T
    u[1] = g_nn(lw.Wqk, D, lw.dT1, D, sl + (2 * H + 1) * DD, D, D, D, HCp);               // slab 2H+1: Q^T dT1 (all heads' rows)
    u[1].a_kmajor = 1;
    u[2] = g_nn(lw.gqk, HCp, lw.Wqk, D, vs + (H + 1) * D, D, 1, D, HCp);                  // vslab H+1: Q^T dt
    RUN(pfo_gemm_multi_launch(u, 3, sf));
  }
  PFO_REQUIRE(H + 3 <= PFO_RANK1_MAX, "too many heads");
  PfoRank1 r[PFO_RANK1_MAX];
  int nr = 0;
  r[nr].u = lw.gqk; r[nr].v = bv; r[nr].M = HCp; r[nr].N = D; r[nr].out = lw.dWqk; r[nr].ldo = D; ++nr;                    // dQ += dt (x) b
  r[nr].u = lw.db1_f; r[nr].v = bv; r[nr].M = D; r[nr].N = D; r[nr].out = g.w1 + E; r[nr].ldo = E + D; ++nr;               // dW1[:, E:] += db1_f (x) b
  for (int h = 0; h < H; ++h) {                                                                                             // dV_node += b (x) dV_f[C]
    r[nr].u = bv; r[nr].v = lw.dW1ovT_f + ((int64_t)h * Cp + C) * D; r[nr].M = D; r[nr].N = D;
    r[nr].out = lw.dW1ovT + (int64_t)h * CpD; r[nr].ldo = D; ++nr;
  }
  RUN(pfo_rank1_multi_launch(r, nr, sf));
  PfoSumSlabs q[3];
  q[0].dst = gp.w2; q[0].src = sl; q[0].stride = DD; q[0].count = DD; q[0].n_slabs = 2 * H + 2;                             // dA
  q[1].dst = gp.b2; q[1].src = vs; q[1].stride = D; q[1].count = D; q[1].n_slabs = H + 2;                                   // db
  q[2].dst = g.b1; q[2].src = lw.db1_f; q[2].stride = 0; q[2].count = D; q[2].n_slabs = 1;                                  // db1 += db1_f
  RUN(pfo_sum_slabs_launch(q, 3, sf));
  PfoRank1 ta;                                                                                                              // dA += sum_h t_node (x) gqk_f,node
  ta.u = lw.tq; ta.v = lw.gqk_f; ta.M = D; ta.N = D; ta.out = gp.w2; ta.ldo = D; ta.reps = H; ta.u_rs = Cp; ta.v_rs = Cp;
  return pfo_rank1_multi_launch(&ta, 1, sf);
}

// Stage 7: the composite-weight gradients chained back to the parameters (tiny products, side streams).
// Half A hangs off dW1ovT (the weight gradients over the instances), half B off dWqk / gqk (those over the table rows).
// At layer 1 the two sources finish ~100 us apart on the side stream, so half A gets a stream of its own and is done
// before half B starts.
static int chain_composites(const Step& S, int l) {
  const Ws& w = S.w; Side& sd = S.sd;
  const LayerWs& lw = w.layer[l];
  const auto& p = S.P.l[l];
  const auto& g = S.G.l[l];
  const int L = S.d.L, D = S.d.D, H = S.d.H, E = S.d.E, C = S.d.C, Cp = S.d.Cp, dh = S.d.dh;
  PfoGemm ca[3], cb[3], c2[3];
  ca[0] = g_nn(p.wv, C, lw.dW1ovT, D, lw.dW1oT, D, dh, D, C);                          // dW1oT_h = Wv_h dW1ovT_h
  ca[0].batch = H; ca[0].a_bs[0] = (int64_t)dh * C; ca[0].b_bs[0] = (int64_t)Cp * D; ca[0].c_bs = (int64_t)dh * D;
  ca[1] = g_nt(lw.W1oT, D, nullptr, lw.dW1ovT, D, g.wv, C, dh, C, D, nullptr);          // dWv_h += W1oT_h dW1ovT_h^T
  ca[1].batch = H; ca[1].a_bs[0] = (int64_t)dh * D; ca[1].b_bs[0] = (int64_t)Cp * D; ca[1].c_bs = (int64_t)dh * C;
  ca[1].accumulate = 1;
  ca[2] = g_nt(lw.W1oT, D, nullptr, lw.dW1ovT + (int64_t)C * D, D, g.b_in + 2 * E, 1, dh, 1, D, nullptr);   // dbv_h += W1oT_h du_h
  ca[2].batch = H; ca[2].a_bs[0] = (int64_t)dh * D; ca[2].b_bs[0] = (int64_t)Cp * D; ca[2].c_bs = dh;
  ca[2].accumulate = 1;
  cb[0] = g_nt(p.wq, E, nullptr, lw.dWqk, D, g.wk, C, dh, C, D, nullptr);               // dWk_h += Wq_h[:, :D] dWqk_h^T
  cb[0].batch = H; cb[0].a_bs[0] = (int64_t)dh * E; cb[0].b_bs[0] = (int64_t)Cp * D; cb[0].c_bs = (int64_t)dh * C;
  cb[0].accumulate = 1;
  cb[1] = g_nn(p.wk, C, lw.dWqk, D, g.wq, E, dh, D, C);                                 // dWq_h[:, :D] += Wk_h dWqk_h
  cb[1].batch = H; cb[1].a_bs[0] = (int64_t)dh * C; cb[1].b_bs[0] = (int64_t)Cp * D; cb[1].c_bs = (int64_t)dh * E;
  cb[1].accumulate = 1;
  cb[2] = g_nt(p.wk, C, nullptr, lw.gqk, C, lw.gq, 1, dh, 1, C, nullptr);                // d cq_h = Wk_h gqk_h
  cb[2].batch = H; cb[2].a_bs[0] = (int64_t)dh * C; cb[2].b_bs[0] = Cp; cb[2].c_bs = dh;
  const float* dc = lw.dW1ovT + (int64_t)(C + 1) * D;                                   // gradient of (W1 bo)^T
  c2[0] = g_nt(lw.dW1oT, D, nullptr, p.wo, E, g.w1, E + D, D, E, E, nullptr);           // dW1[:, :E] += dW1o Wo^T
  c2[0].a_kmajor = 1; c2[0].accumulate = 1;
  c2[1] = g_nt(p.w1, E + D, nullptr, lw.dW1oT, D, g.wo, E, E, E, D, nullptr);           // dWo += W1[:, :E]^T dW1o
  c2[1].a_kmajor = 1; c2[1].accumulate = 1;
  c2[2] = g_nt(p.w1, E + D, nullptr, dc, D, g.bo, 1, E, 1, D, nullptr);                // dbo += W1[:, :E]^T dc
  c2[2].a_kmajor = 1; c2[2].accumulate = 1;
  // the outer-product halves of the composite gradients, one launch per half (disjoint outputs):
  //   A: W1ovT row C = bv_h^T W1oT_h (into dW1oT, which c2 reads),  dW1[:, :E] += dc (x) bo     B: cqk_h = Wk_h^T cq_h
  PFO_REQUIRE(H + 1 <= PFO_RANK1_MAX, "too many heads");
  PfoRank1 ra[PFO_RANK1_MAX], rb[PFO_RANK1_MAX];
  for (int h = 0; h < H; ++h) {
    ra[h].u = p.b_in + 2 * E + h * dh; ra[h].ldu = 1; ra[h].v = lw.dW1ovT + ((int64_t)h * Cp + C) * D; ra[h].ldv = 1;
    ra[h].M = dh; ra[h].N = D; ra[h].out = lw.dW1oT + (int64_t)h * dh * D; ra[h].ldo = D;
    rb[h].u = lw.cq + h * dh; rb[h].ldu = 1; rb[h].v = lw.gqk + (int64_t)h * Cp; rb[h].ldv = 1;
    rb[h].M = dh; rb[h].N = C; rb[h].out = g.wk + (int64_t)h * dh * C; rb[h].ldo = C;
  }
  ra[H].u = dc; ra[H].ldu = 1; ra[H].v = p.bo; ra[H].ldv = 1; ra[H].M = D; ra[H].N = E; ra[H].out = g.w1; ra[H].ldo = E + D;
  hipStream_t sa = S.s2, sb = S.s2;
  if (l == 1) {
    // both sources were launched on side streams (or, bracketed for profiling, the first on the main stream): no need to
    // hold the chain behind the main stream's d h0 contraction
    sb = S.ss;
    HIPOK(hipStreamWaitEvent(sa, sd.tn_a_done, 0), "event wait failed");
  }
  if (l == 1) PFO_MARK("@side2.L1.chainA.begin", sa);
  RUN(pfo_gemm_multi_launch(ca, 3, sa));
  RUN(pfo_rank1_multi_launch(ra, H + 1, sa));
  RUN(pfo_gemm_multi_launch(c2, 3, sa));
  if (l == 1) PFO_MARK("@side2.L1.chainA.end", sa);
  else PFO_MARK("@side2.L2.chainA.end", sa);
  RUN(pfo_gemm_multi_launch(cb, 3, sb));
  RUN(pfo_rank1_multi_launch(rb, H, sb));
  if (l == 1) PFO_MARK("@side1.L1.chainB.end", sb);
  else PFO_MARK("@side2.L2.chainB.end", sb);
  if (l == L && L >= 2) {
    // The top layer's folded query-bias backward runs here, on the stream of its chain, with its time-bias term parked in
    // tb_part (the final launch adds it): from this point every gradient of the top layer's parameter block
    // [layer[L-1].wq, total) is FINAL - a data-parallel caller starts all-reducing that block while layers L-1 .. 1 are
    // still being differentiated (pfo_tgn_grad_split, distributed.py)
    const float* gq1[1] = {lw.gq}; const float* wq1[1] = {p.wq};
    float* dbq1[1] = {g.b_in}; float* dwq1[1] = {g.wq};
    RUN(pfo_cq_backward_launch(gq1, wq1, 1, S.P.tb, D, dbq1, dwq1, S.G.tb, w.tb_part, nullptr, nullptr, 0, nullptr, sb));
    if (S.top_ready_event) HIPOK(hipEventRecord((hipEvent_t)S.top_ready_event, sb), "event record failed");
  }
  return PFO_OK;
}
// ~15 launches that no launch of the caller's stream waits for (stages 6 and 7 of one layer)
static int chain_back(const Step& S, const Chain& ch) {
  if (ch.l >= 2) RUN(unfold_fc2(S, ch));
  return chain_composites(S, ch.l);
}

// Stage 8: GRU parameters (messages and stored memory are constants: SURVEY App. A-6)
static int backward_gru(const Step& S, bool* main_done_bound) {
  PfoRange range_gru("backward GRU");
  const Ws& w = S.w;
  const int D = S.d.D, M = S.d.M;
  // (the GRU's backward covers the rows the layers read: rows only the extra list names carry no gradient)
  RUN(pfo_gru_gates_bwd_launch(w.gates, w.gi, w.gh, w.h_rows, w.hm, w.n_core, S.capP, D, w.d_h0, S.n_rep, S.rep_stride,
                               w.dx_tab, S.det, S.s));
  PFO_MARK("bwd.gru.gates", S.s);
  PfoTnProblem gp[4];
  int ngp = 2;
  gp[0] = tn_of(w.gi, 3 * D, w.msg_rows, M, nullptr, 3 * D, M, S.G.w_ih, M, S.G.b_ih);
  gp[1] = tn_of(w.gh, 3 * D, w.h_rows, D, nullptr, 3 * D, D, S.G.w_hh, D, S.G.b_hh);
  if (S.d.Hm > 0) {
    // the MLP message function's data path: d m = dgi W_ih, d hid = (d m W2) where hid > 0; then its two weight gradients
    // join the GRU's group (dW_ih now contracts against the MLP's output rows)
    const int Mg = S.d.Mg, Hm = S.d.Hm;
    PfoGemm q1 = g_nn(w.gi, 3 * D, S.P.w_ih, Mg, w.d_m, Mg, S.capP, Mg, 3 * D);
    q1.m_dev = w.n_core; q1.b_img = w.iWihT;
    RUN(pfo_gemm_launch(q1, S.s));
    PfoGemm q2 = g_nn(w.d_m, Mg, S.P.m_w2, Hm, w.d_hid, Hm, S.capP, Hm, Mg);
    q2.m_dev = w.n_core; q2.b_img = w.iMW2T; q2.relu_src = w.mlp_hid; q2.relu_ld = Hm;
    RUN(pfo_gemm_launch(q2, S.s));
    PFO_MARK("bwd.msg_mlp", S.s);
    gp[0] = tn_of(w.gi, 3 * D, w.mlp_out, Mg, nullptr, 3 * D, Mg, S.G.w_ih, Mg, S.G.b_ih);
    gp[2] = tn_of(w.d_m, Mg, w.mlp_hid, Hm, nullptr, Mg, Hm, S.G.m_w2, Hm, S.G.m_b2);
    gp[3] = tn_of(w.d_hid, Hm, w.msg_rows, M, nullptr, Hm, M, S.G.m_w1, M, S.G.m_b1);
    ngp = 4;
  }
  // (a deferred join's main_done event rides on the slab reduce, the caller's stream's last launch of this call)
  *main_done_bound = S.b->defer_join && !S.capturing;
  PFO_RUN_BOUND(*main_done_bound, S.sd.main_done, 1, S.s, pfo_gemm_tn_group_launch(gp, ngp, S.capP, w.n_core, w.slabs, w.slab_floats, S.s));
  PFO_MARK("bwd.gru.tn", S.s);
  return PFO_OK;
}

// Stage 9: the last small launches go to the first side stream, beside the GRU's weight gradients on the caller's stream:
// [deterministic mode: the attention backwards' slab rows fold, in row order, into bin 0 of the (otherwise empty) fp64 bins]
// then ONE launch finishes the time-encoder gradients: the folded query-bias backward of layers 1 .. L-1 (the top layer's ran
// with its chain), + its parked time-bias term, + the fold of the fp64 partial sums into time_w / time_b (fixed order).
// That stream has seen every attention backward (it waited for tn_b, recorded behind layer 1's) and runs layer 1's chain.
// Then the closing join.
static int backward_close(const Step& S, bool main_done_bound) {
  const Ws& w = S.w; Side& sd = S.sd;
  hipStream_t s = S.s, ss = S.ss;
  const int L = S.d.L, D = S.d.D;
  const bool chained = !S.capturing;
  // The side streams are joined in a chain - the first waits for the second, the caller's stream for the first: one wait on
  // the critical path instead of two - except while the caller's stream is being captured into a HIP graph, where that
  // topology makes hipStreamEndCapture of ROCm 7.0 segfault: there the caller's stream waits for both itself.
  HIPOK(hipEventRecord(sd.done2, S.s2), "event record failed");
  HIPOK(hipStreamWaitEvent(chained ? ss : s, sd.done2, 0), "event wait failed");
  if (!chained) {                                             // (the launches below read the second side stream's results)
    HIPOK(hipEventRecord(sd.tn_a, s), "event record failed");
    HIPOK(hipStreamWaitEvent(ss, sd.tn_a, 0), "event wait failed");
  }
  if (S.det) RUN(pfo_fold_parts_launch(w.dtime_slab, (int)S.det_rows, 2 * D, nullptr, 0, w.fold_scratch, w.tickets, ss, w.dtime));
  const float *gq[PFO_MAX_LAYERS], *wq[PFO_MAX_LAYERS];
  float *dbq[PFO_MAX_LAYERS], *dwq[PFO_MAX_LAYERS];
  const int nl = L >= 2 ? L - 1 : L;
  for (int l = 1; l <= nl; ++l) { gq[l - 1] = w.layer[l].gq; wq[l - 1] = S.P.l[l].wq; dbq[l - 1] = S.G.l[l].b_in; dwq[l - 1] = S.G.l[l].wq; }
  RUN(pfo_cq_backward_launch(gq, wq, nl, S.P.tb, D, dbq, dwq, S.G.tb, nullptr, L >= 2 ? w.tb_part : nullptr, w.dtime,
                             pfo_attn_bwd_max_parts(), S.G.tw, ss));                  // cq = Wq[:, D:] cos(b) + bq
  PFO_MARK("@side1.cq.end", ss);
  if (S.b->defer_join && chained) {                            // (not under capture - side_join)
    // the end of the backward stays on the side stream (pfo_tgn_batch.defer_join): it waits for the caller's stream's last
    // launch instead of the other way round - the caller's stream is free for the next batch's neighbour sampling
    if (!main_done_bound) HIPOK(hipEventRecord(sd.main_done, s), "event record failed");
    HIPOK(hipStreamWaitEvent(ss, sd.main_done, 0), "event wait failed");
    sd.side_gen += 1;
    sd.last_backward_deferred = true;
    sd.deferred_from = s;
  } else {
    sd.last_backward_deferred = false;
    sd.deferred_from = nullptr;
    HIPOK(hipEventRecord(sd.done, ss), "event record failed");
    HIPOK(hipStreamWaitEvent(s, sd.done, 0), "event wait failed");
  }
  return PFO_OK;
}

extern "C" int pfo_tgn_backward(const pfo_tgn_config* c, const pfo_tgn_state* st, const pfo_tgn_batch* b, void* workspace,
                                const float* d_emb, float* grad, void* stream) {
  return pfo_tgn_backward_ev(c, st, b, workspace, d_emb, grad, 0, nullptr, nullptr, 0, nullptr, stream);
}

extern "C" int pfo_tgn_backward_ev(const pfo_tgn_config* c, const pfo_tgn_state* st, const pfo_tgn_batch* b, void* workspace,
                                   const float* d_emb, float* grad, int32_t zero_grad_first, void* top_ready_event,
                                   const float* mean_src, int64_t mean_n, float* mean_out, void* stream) {
  if (int rc = check_cfg(c)) return rc;
  PFO_REQUIRE(st && workspace && d_emb && grad && st->params, "null argument");
  PFO_REQUIRE(!mean_src || (mean_n > 0 && mean_out), "bad deferred mean");
  Step S(side());
  RUN(open_step(S, c, st, b, workspace, stream));      // (the composites and images the forward used)
  bind(S.lay, grad, S.G, S.d.L, c->use_memory != 0);
  S.d_emb = d_emb; S.top_ready_event = top_ready_event;
  S.mean_src = mean_src; S.mean_n = mean_n; S.mean_out = mean_out;
  S.seg_fwd = b->seg_in_forward && b->upd_src != nullptr && c->use_memory && S.d.L >= 2;

  PfoRange range_call("pfo_tgn_backward");
  PFO_REQUIRE(S.sd.ok, "could not create the side stream");
  RUN(side_join(S.sd, S.s));
  PFO_MARK("bwd.begin", S.s);
  // (the gradient buffer is cleared on the caller's stream, before the fork: every writer on any stream comes after it)
  if (zero_grad_first) HIPOK(hipMemsetAsync(grad, 0, (size_t)S.lay.total * sizeof(float), S.s), "memset failed");
  RUN(backward_open(S));
  // A layer's chain back to the parameters: for a layer >= 2 the HOST issues it only after the next layer's data-gradient
  // launches are queued (r3 timeline: the caller's stream sat idle for ~60 us behind them while the host was the slower side);
  // the event that releases it on the device (layer[l]) stays where it was.  (Layer 1 never waits: nothing is left pending.)
  Chain pending;
  for (int l = S.d.L; l >= 1; --l) {
    PfoRange range_layer(LAYER_NAMES[NM_BWD][l]);
    LayerBack lb;
    lb.v = layer_view(S, l);
    lb.ch.l = l;
    if (l == S.d.L) RUN(backward_top_dh1(S, lb));
    else lb.dh1 = S.w.dH[l];
    RUN(backward_dctx(S, lb));
    RUN(backward_attn(S, lb));
    if (pending.l) { RUN(chain_back(S, pending)); pending.l = 0; }     // the layer above's chain-back (side streams)
    if (l == 1) RUN(backward_table_side(S, lb));
    else RUN(backward_x_side(S, lb));
    if (l > 1 && !pfo_prof_on()) pending = lb.ch;
    else RUN(chain_back(S, lb.ch));
  }
  bool main_done_bound = false;
  if (c->use_memory) RUN(backward_gru(S, &main_done_bound));
  RUN(backward_close(S, main_done_bound));
  PFO_MARK("bwd.end", S.s);
  return PFO_OK;
}


int pfo_adam_step_ranges_impl(float*, float*, float*, float*, int32_t, const int64_t*, const int64_t*, const int32_t*, float, float, float,
                              float, bool, void*);
static int adam_side_impl(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int32_t n_ranges,
                          const int64_t* lo, const int64_t* hi, const int32_t* step, float lr, float beta1, float beta2,
                          float eps, bool zero_grad) {
  Side& sd = side();
  PFO_REQUIRE(sd.ok, "could not create the side stream");
  PFO_REQUIRE(sd.last_backward_deferred, "pfo_tgn_adam_side follows a backward that ran with pfo_tgn_batch.defer_join");
  const int rc = pfo_adam_step_ranges_impl(param, grad, exp_avg, exp_avg_sq, n_ranges, lo, hi, step, lr, beta1, beta2, eps, zero_grad, (void*)sd.s);
  sd.side_gen += 1;                                              // (a stream that joined between the backward and this call joins again)
  PFO_MARK("@side1.adam.end", sd.s);
  return rc;
}
extern "C" int pfo_tgn_adam_side(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int32_t n_ranges,
                                 const int64_t* lo, const int64_t* hi, const int32_t* step, float lr, float beta1, float beta2,
                                 float eps) {
  return adam_side_impl(param, const_cast<float*>(grad), exp_avg, exp_avg_sq, n_ranges, lo, hi, step, lr, beta1, beta2, eps, false);
}

extern "C" int pfo_tgn_adam_side_bucket(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int32_t n_ranges,
                                        const int64_t* lo, const int64_t* hi, const int32_t* step, float lr, float beta1, float beta2,
                                        float eps, int32_t flags) {
  Side& sd = side();
  PFO_REQUIRE(sd.ok, "could not create the side stream");
  const int bucket = flags & 3;
  PFO_REQUIRE(flags >= 0 && flags < 8 && bucket <= 2, "flags: bucket 0 (plain), 1 (first use) or 2 (later bucket of the same step), + 4 = clear the gradient ranges");
  PFO_REQUIRE(bucket != 2 || sd.early_ok, "a later bucket follows a first-use bucket of the same step");
  const int rc = adam_side_impl(param, grad, exp_avg, exp_avg_sq, n_ranges, lo, hi, step, lr, beta1, beta2, eps, (flags & 4) != 0);
  if (rc != PFO_OK) { sd.early_ok = false; return rc; }
  if (bucket == 1) {
    HIPOK(hipEventRecord(sd.early_done, sd.s), "event record failed");
    sd.early_ok = true;
  }
  if (bucket == 0) sd.early_ok = false;
  sd.early_gen = sd.side_gen;                                    // (bucket 2: the event of bucket 1 still stands for the stream's tail)
  return PFO_OK;
}

extern "C" void* pfo_tgn_side_stream(void) {
  Side& sd = side();
  if (!sd.ok) { pfo_set_error("pfo_tgn_side_stream: could not create the side stream"); return nullptr; }
  return (void*)sd.s;
}

extern "C" int pfo_tgn_join(void* stream) {
  Side& sd = side();
  PFO_REQUIRE(sd.ok, "could not create the side stream");
  return side_join(sd, (hipStream_t)stream);
}

// =============================================================================================
extern "C" int pfo_tgn_update_state(const pfo_tgn_config* c, const pfo_tgn_state* st, const int32_t* src,
                                    const int32_t* dst, const double* ts, const int32_t* eidx, int32_t B, void* workspace,
                                    void* stream) {
  if (int rc = check_cfg(c)) return rc;
  if (!c->use_memory) return PFO_OK;
  PFO_REQUIRE(st && workspace && src && dst && ts && eidx && B >= 1, "bad arguments");
  const Ws w = carve(c, workspace);
  PfoRange range("pfo_tgn_update_state");
  RUN(side_join(side(), (hipStream_t)stream));
  return state_update(c, st, w, src, dst, ts, eidx, B, (hipStream_t)stream);
}

// =============================================================================================
// The serving write path: a chronological log walked in batches of B, the model state left where the step would leave it -
// without sampling, attention or embeddings (tgn.py:295-317 alone).  Per batch four launches on the caller's stream
// (five beyond MSG_INLINE_MAX events): row selection (memory.hip observe_select_kernel) -> the step's own fused GRU in its
// gather form over exactly those rows -> persist -> [winner pass] -> message store; the last three are state_update().
// The GRU result goes through the packed buffer + persist_kernel, not an in-place epilogue: gru_fused_kernel and
// state_update() are then the training step's, launched unchanged - the parity with the step is shared code.
namespace {
struct ObsWs {
  int32_t *rep, *slot, *touched, *n_rows, *winner;
  float *upd_mem, *h0_tab, *gates;
  void *iWih, *iWhh;
  float *mlp_hid, *mlp_out;                 // message MLP (msg_dim > 0)
  void *iMW1, *iMW2;
  int64_t cap, bytes;
};
ObsWs carve_observe(const pfo_tgn_config* c, int32_t B, void* base) {
  const Dims d = dims_of(c);
  ObsWs o;
  memset(&o, 0, sizeof(o));
  char* p = reinterpret_cast<char*>(base);
  o.cap = std::min<int64_t>(c->n_nodes, 2 * (int64_t)B);          // distinct positives of one batch
  o.rep = take<int32_t>(p, c->n_nodes);
  o.slot = take<int32_t>(p, c->n_nodes);
  o.touched = take<int32_t>(p, o.cap);
  o.n_rows = take<int32_t>(p, 64);
  if (pfo_msg_store_needs_winner(B)) o.winner = take<int32_t>(p, c->n_nodes);
  o.upd_mem = take<float>(p, o.cap * d.D);
  o.h0_tab = take<float>(p, o.cap * d.D);                         // (by-products of the fused launch, not read here)
  o.gates = take<float>(p, o.cap * 4 * d.D);
  o.iWih = take<char>(p, pfo_gru_img_bytes(d.D, d.Mg));           // (used when the state carries no valid parameter cache)
  o.iWhh = take<char>(p, pfo_gru_img_bytes(d.D, d.D));
  if (d.Hm > 0) {
    o.mlp_hid = take<float>(p, o.cap * d.Hm);
    o.mlp_out = take<float>(p, o.cap * d.Mg);
    o.iMW1 = take<char>(p, pfo_bimg_bytes(d.Hm, d.M));
    o.iMW2 = take<char>(p, pfo_bimg_bytes(d.Mg, d.Hm));
  }
  o.bytes = p - reinterpret_cast<char*>(base);
  return o;
}
int check_observe(const pfo_tgn_config* c, int32_t B) {
  if (int rc = check_cfg(c)) return rc;
  PFO_REQUIRE(c->use_memory != 0, "a model without memory has no state to advance");
  PFO_REQUIRE(B >= 1 && B < (1 << 30), "B must be in [1, 2^30)");
  return PFO_OK;
}
}  // namespace

extern "C" int64_t pfo_tgn_observe_workspace_bytes(const pfo_tgn_config* c, int32_t B) {
  if (check_observe(c, B) != PFO_OK) return -1;
  return carve_observe(c, B, nullptr).bytes + 256;
}

extern "C" int pfo_tgn_observe(const pfo_tgn_config* c, const pfo_tgn_state* st, const int32_t* src, const int32_t* dst,
                               const double* ts, const int32_t* eidx, int64_t N, int32_t B, void* workspace,
                               int64_t workspace_bytes, void* stream) {
  if (int rc = check_observe(c, B)) return rc;
  PFO_REQUIRE(N >= 0, "N must not be negative");
  if (N == 0) return PFO_OK;
  PFO_REQUIRE(workspace_bytes >= carve_observe(c, B, nullptr).bytes + 256, "workspace too small (pfo_tgn_observe_workspace_bytes)");
  PFO_REQUIRE(st && workspace && src && dst && ts && eidx, "null argument");
  PFO_REQUIRE(st->node_feat && st->params && st->memory && st->last_update && st->msg_table && st->msg_time && st->has_msg, "null state");
  PFO_REQUIRE(c->Ef == 0 || st->edge_feat, "null edge features");
  const Dims d = dims_of(c);
  const ObsWs o = carve_observe(c, B, reinterpret_cast<void*>(pfo_align_up((int64_t)(uintptr_t)workspace, 256)));
  hipStream_t s = (hipStream_t)stream;
  pfo_tgn_layout lay;
  RUN(pfo_tgn_param_layout(c, &lay));
  Params P;
  bind(lay, st->params, P, d.L, true);
  PfoRange range("pfo_tgn_observe");
  RUN(side_join(side(), s));                                      // (a deferred optimizer step may still be writing the parameters)
  // GRU weight images: the parameter cache's when it is valid, else built here, once - parameters cannot change inside a call
  const void *iWih = o.iWih, *iWhh = o.iWhh, *iMW1 = o.iMW1, *iMW2 = o.iMW2;
  if (st->pcache && st->pcache_valid) {
    const Ws pw = carve(c, nullptr, st->pcache, true);
    iWih = pw.iWih; iWhh = pw.iWhh; iMW1 = pw.iMW1; iMW2 = pw.iMW2;
  } else {
    Ws bw;
    memset(&bw, 0, sizeof(bw));
    bw.iWih = o.iWih; bw.iWhh = o.iWhh; bw.iMW1 = o.iMW1; bw.iMW2 = o.iMW2;
    RUN(build_gru_images(c, d, bw, P, s, true));
  }
  HIPOK(hipMemsetAsync(o.rep, 0, (size_t)c->n_nodes * sizeof(int32_t), s), "memset failed");
  Ws w;                                                           // what state_update() reads of a step's workspace
  memset(&w, 0, sizeof(w));
  w.slot = o.slot; w.upd_mem = o.upd_mem; w.winner = o.winner;
  int64_t base = 0;
  for (int64_t k0 = 0; k0 < N; k0 += B) {
    const int32_t b = (int32_t)std::min<int64_t>(B, N - k0);
    if (base + 2 * (int64_t)b >= 0x7fffffffll) {                  // the stamps would leave int32: start over on a cleared table
      HIPOK(hipMemsetAsync(o.rep, 0, (size_t)c->n_nodes * sizeof(int32_t), s), "memset failed");
      base = 0;
    }
    RUN(pfo_observe_select_launch(src + k0, dst + k0, b, st->has_msg, o.rep, (int)base, o.slot, o.touched, o.n_rows, s));
    base += 2 * (int64_t)b;
    PfoGruFused f;
    f.gather = 1; f.msg_rows = st->msg_table; f.K_msg = d.Mg; f.h_rows = st->memory; f.hm = st->has_msg;
    f.img_ih = iWih; f.img_hh = iWhh; f.b_ih = P.b_ih; f.b_hh = P.b_hh; f.touched = o.touched; f.node_feat = st->node_feat;
    f.upd_mem = o.upd_mem; f.h0_tab = o.h0_tab; f.gates = o.gates; f.D = d.D;
    f.cap_rows = (int)std::min<int64_t>(c->n_nodes, 2 * (int64_t)b); f.n_rows = o.n_rows;
    if (d.Hm > 0) {                                               // the step's own MLP stage over the selected rows
      RUN(message_mlp(d, P, st->msg_table, o.touched, iMW1, iMW2, o.mlp_hid, o.mlp_out, f.cap_rows, o.n_rows, s));
      f.gather = 2; f.msg_rows = o.mlp_out;
    }
    RUN(pfo_gru_fused_launch(f, s));
    RUN(state_update(c, st, w, src + k0, dst + k0, ts + k0, eidx + k0, b, s));
  }
  return PFO_OK;
}
