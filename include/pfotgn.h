/*
 * pfotgn.h - C ABI of the MI355X-native TGN-recommender training path.
 *
 * Drop-in boundary for the hot path of youngandbin/PfoTGNRec (reference is pure
 * Python; citations are file:line under /root/reference).  Every entry point takes
 * plain DEVICE pointers (unless marked host), sizes and a hipStream_t passed as
 * void*; no torch / C++ types cross this boundary.  All kernels are gfx950 HIP.
 *
 * Conventions
 *   - return value: 0 = ok, <0 = error (pfo_last_error() gives the message, per thread)
 *   - node / edge ids on device are int32 (node 0 and edge 0 are padding)
 *   - all floating-point tensors are fp32 row-major unless stated (timestamps fp64)
 *   - nothing here allocates, frees or synchronises: callers own every buffer
 */
#ifndef PFOTGN_H
#define PFOTGN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFO_OK 0
#define PFO_ERR_INVALID (-1)
#define PFO_ERR_HIP (-2)

#define PFO_MAX_NEIGHBORS 64 /* K: one wavefront lane per neighbour slot */
#define PFO_MAX_LAYERS 4
#define PFO_MAX_HEADS 8

int pfo_abi_version(void);
const char* pfo_last_error(void);

/* ------------------------------------------------------------------------------------------
 * K1  temporal neighbour lookup over a time-sorted CSR.
 * Replaces NeighborFinder.find_before + get_temporal_neighbor (utils/utils.py:150-219).
 *
 *   indptr  i64[n_nodes+1]; adj_nbr i32[nnz]; adj_eidx i32[nnz]; adj_ts f64[nnz] (per node ascending,
 *   ties in edge order - what utils/utils.py:139 `sorted(key=ts)` yields).
 *   Query i = (q_nodes[i], q_ts[i]); entries with ts STRICTLY < q_ts qualify (searchsorted side='left').
 *   mode 0: most-recent K, right-aligned, left-padded with (0,0,0.0)              (:206-218)
 *   mode 1: uniform with INJECTED draws  draws i64[n_q,K] in [0, #qualifying)     (:194)
 *   mode 2: uniform with counter-based Philox draws (seed, stream offset)
 *   uniform modes re-sort each row by f32 time, STABLE (tie policy SURVEY App. A-9)   (:201-204)
 *   K == 0 is treated as one all-padding column by the host mirror (:175); here K >= 1.
 * Outputs (any may be NULL): out_nbr/out_eidx i32[n_q,K], out_et f32[n_q,K] (edge time cast to f32),
 *   out_dt f32[n_q,K] = f32( q_ts - f64(out_et) )  (embedding_module.py:133-135).
 * Frontier expansion (optional, next_nodes != NULL): writes the next recursion level
 *   next_nodes[0:n_q] = q_nodes, next_nodes[n_q + i*K + j] = nbr[i][j]; next_ts (optional) likewise, q_ts[i] repeated
 *   (embedding_module.py:115,141-145: neighbours are evaluated at the ROOT's timestamp).
 */
int pfo_tnbr_sample(const int64_t* indptr, const int32_t* adj_nbr, const int32_t* adj_eidx, const double* adj_ts,
                    int64_t n_nodes, const int32_t* q_nodes, const double* q_ts, int64_t n_q, int32_t K,
                    int32_t mode, const int64_t* draws, uint64_t seed, uint64_t offset,
                    int32_t* out_nbr, int32_t* out_eidx, float* out_et, float* out_dt,
                    int32_t* next_nodes, double* next_ts, void* stream);

/* ------------------------------------------------------------------------------------------
 * Candidate-negative draw.  Replaces RandEdgeSampler.sample (utils/utils.py:86-114).
 *   item_avail u8[n_items]: 1 if the item occurs among the train destinations (np.unique(dst_list), :73)
 *   port_idx i32[B,port_stride] 0-based item indices, port_len i32[B] (the '' entry is already dropped, :76)
 *   out i32[B,size] = item NODE ids (index + upper_u + 1), drawn without replacement from
 *   avail \ portfolio when that set has >= size members, otherwise with replacement (:99-111).
 *   RNG: Philox(seed, offset + interaction) - semantics-level parity only.
 *   The draw itself (DESIGN "Random streams"; pinned bit for bit by tests/philox_ref.py): row b's list = the available items
 *   in ascending index that are not among its first min(port_len, port_stride) portfolio entries (entries outside
 *   [0, n_items) exclude nothing); slot k reads word k & 3 of the Philox4x32-10 block at counter (b + offset, k >> 2);
 *   n_avail >= size: step k of a partial Fisher-Yates swaps entry k with entry k + ((word * (n_avail - k)) >> 32) and emits it;
 *   0 < n_avail < size: list[(word * n_avail) >> 32]; n_avail == 0: the row is all ZEROS (node id 0, the padding node).
 *   1 <= n_items <= 16384: the list lives in n_items * 4 bytes of dynamic LDS, 64 KiB at the maximum.
 */
int pfo_neg_draw(const uint8_t* item_avail, int32_t n_items, const int32_t* port_idx, const int32_t* port_len,
                 int32_t port_stride, int64_t B, int32_t size, int32_t upper_u, uint64_t seed, uint64_t offset,
                 int32_t* out, void* stream);
/* the same with a device word added to `offset` (graph-captured steps, see pfo_tgn_batch.offset_dev) */
int pfo_neg_draw_dev(const uint8_t* item_avail, int32_t n_items, const int32_t* port_idx, const int32_t* port_len,
                     int32_t port_stride, int64_t B, int32_t size, int32_t upper_u, uint64_t seed, uint64_t offset,
                     const uint64_t* offset_dev, int32_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * K2  mean-variance-efficient rank fusion.  Replaces the inline block main.py:209-304.
 *   returns f64[n_days,n_items,n_ret]: log-returns log(p[t+1]/p[t]) (main.py:218,226-227; n_ret = 29)
 *   day_idx i32[B]; cand i32[B,n_cand] item NODE ids, column 0 = true destination (main.py:207)
 *   y_mv = (mu/gamma - 0.5*mean_j cov_ij)/cov_ii, or (mu/gamma)/var_i for an empty portfolio (main.py:243-271)
 *   invest_rank = average-tie rank of y_mv; tgn_rank = n..1; new = lam*invest + (1-lam)*tgn (main.py:282-286)
 *   order = stable ascending argsort of new, reversed (tie policy SURVEY App. A-9; main.py:289)
 *   p_pos i32[B,n_pos] = first n_pos of order, p_neg i32[B,n_neg] = last n_neg (main.py:291-292), as node ids.
 *   y_out f64[B,n_cand] and rank_out f64[B,n_cand] (new_rank) are optional diagnostics.
 */
int pfo_mv_select(const double* returns, int32_t n_days, int32_t n_items, int32_t n_ret, const int32_t* day_idx,
                  const int32_t* cand, int32_t n_cand, const int32_t* port_idx, const int32_t* port_len,
                  int32_t port_stride, int64_t B, int32_t upper_u, double gamma, double lambda_mv,
                  int32_t n_pos, int32_t n_neg, int32_t* p_pos, int32_t* p_neg, double* y_out, double* rank_out,
                  void* stream);

/* ------------------------------------------------------------------------------------------
 * TimeEncode forward: out[i,d] = cos(fma(t[i], w[d], b[d]))   (model/time_encoding.py:17-25;
 * single fp32 FMA then a full-range cosine - SURVEY §7 hard part 1).
 */
int pfo_time_encode(const float* t, int64_t n, const float* w, const float* b, int32_t D, float* out, void* stream);

/* The train-mode dropout multipliers of one attention layer, exactly as the step's kernels draw them
 * (nn.MultiheadAttention(dropout=p) on the softmax weights, temporal_attention.py:28,70): out[n, h, j] = 1/(1-p) where the
 * weight of key slot j / head h of instance n is kept, 0 where it is dropped.  Philox4x32 keyed by `seed`, counter
 * (n * 64 + j, offset): the step uses offset = pfo_tgn_batch.offset + 0x51ED0000 + layer (1-based), n = the instance's index
 * in the layer's level list.  Test / parity infrastructure: lets an oracle replay a dropout-0.1 step with the SAME masks
 * (the RNG stream itself is not part of the reference's contract). */
int pfo_attn_dropout_mask(uint64_t seed, uint64_t offset, int64_t N, int32_t K, int32_t H, float p, float* out /* [N,H,K] */,
                          void* stream);

/* ------------------------------------------------------------------------------------------
 * Gradient rows of the instances that sit on one node, summed per node: the backward of the reference's reuse of one
 * level-0 row [memory + features] by every instance of that node (embedding_module.py:93-98, the index by node id there;
 * autograd's index backward is this sum).  Exposed for tests; the step calls it between layer 1's attention backward and
 * the touched-table contraction.
 *   out[s, :] = sum over m in [seg_ptr[s], seg_ptr[s+1]) of [ src0[p(m), 0:W0] | src1[members[m], 0:W1] ],  s < *n_rows
 *   p(m) = m (src0_by_position != 0: rows stored in member order) or members[m]
 *   src0_live (optional, with src0_by_position): byte per position, 0 = that src0 row holds nothing and is not read
 *   seg_of (optional): int32 per member position, the segment it belongs to, in an array of at least
 *   (n_members / 16 + 2) * 16 entries (the tail unused).  With it the launch is cut by members instead of by segments
 *   (balanced whatever the segment lengths); without it, four segments per workgroup.
 * Rows are added in member order: the result is the sequential sum, the same on every run.
 * seg_ptr / members / seg_of / n_rows are device arrays (n_rows: one int32, <= cap_rows; n_members >= seg_ptr[*n_rows]).
 */
int pfo_segment_sum(const float* src0, int32_t W0, const float* src1, int32_t W1, const int32_t* seg_ptr,
                    const int32_t* members, const int32_t* seg_of, int64_t n_members, const int32_t* n_rows,
                    int32_t cap_rows, int32_t src0_by_position, const uint8_t* src0_live,
                    float* out /* [cap_rows, W0+W1] */, void* stream);

/* ------------------------------------------------------------------------------------------
 * Dense fp32 contraction on the matrix cores (v_mfma_f32_16x16x4_f32), exposed for tests.
 *   C[M,N] = A[M,K] * op(B) + bias,  op(B) = B[N,K]^T (b_kmajor = 0, the nn.Linear weight layout)
 *                                    or      B[K,N]   (b_kmajor = 1)
 *   a_kmajor = 1 reads A as [K,M] (used for weight gradients dW = dY^T X).
 */
int pfo_gemm_f32(const float* A, int64_t lda, int32_t a_kmajor, const float* B, int64_t ldb, int32_t b_kmajor,
                 float* C, int64_t ldc, const float* bias, int32_t M, int32_t N, int32_t K, int32_t relu,
                 float* workspace, int64_t workspace_floats, void* stream);

/* ------------------------------------------------------------------------------------------
 * The same contraction for row-major A, computed on the 16-bit matrix cores by splitting every fp32 operand into pieces
 * with exact residuals and accumulating the piece products in fp32: fp32-level accuracy (error <= ~2^-22 sum_k |a||b|,
 * the bound of an fp32 accumulation).  Default: TWO fp16 pieces of the operand times a per-row power of two, x 2^s = h + l,
 * three v_mfma_f32_16x16x32_f16 per block (weight rows scaled from their maximum, activation rows from a running maximum with
 * exact accumulator rescaling; elements below 2^-16 of their row's maximum keep an absolute error <= 2^-38 of that maximum).
 * With PFO_BX_FMT=0 in the environment: THREE bf16 pieces, x = x1 + x2 + x3, six v_mfma_f32_16x16x32_bf16 per block (the
 * symbol's name).  This is the kernel the large launches of pfo_tgn_forward / pfo_tgn_backward use for torch.nn.Linear
 * (utils.py:7-17, torch.nn.MultiheadAttention in temporal_attention.py:27-31); it is exported so that it can be checked alone.
 *   workspace: pfo_gemm_bf16x3_workspace_bytes(N, K) bytes, 16-byte aligned (receives the split image of B).
 *   A 16-byte aligned, lda % 4 == 0, K % 4 == 0.
 */
int64_t pfo_gemm_bf16x3_workspace_bytes(int32_t N, int32_t K);
int pfo_gemm_bf16x3(const float* A, int64_t lda, const float* B, int64_t ldb, int32_t b_kmajor, float* C, int64_t ldc,
                    const float* bias, int32_t M, int32_t N, int32_t K, int32_t relu, void* workspace,
                    int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Root list of one batch shard, the node/timestamp arrays the reference concatenates before compute_embedding
 * (tgn.py:118-124 for the `ours` path, tgn.py:237-239 for the baseline):
 *   roots   = [ src[lo:hi] | dst[lo:hi] | groups[0][lo:hi, :] | groups[1][lo:hi, :] ... ]
 *   root_ts = ts of the interaction each root belongs to (edge_times repeated per group element)
 * groups[g] i32[B * reps[g]] (device pointers in a HOST array of n_groups <= PFO_MAX_ROOT_GROUPS entries), row-major
 * per interaction.  roots i32[R], root_ts f64[R], R = (hi - lo) * (2 + sum reps).
 */
#define PFO_MAX_ROOT_GROUPS 4
int pfo_roots_assemble(const int32_t* src, const int32_t* dst, const double* ts, int32_t lo, int32_t hi,
                       const int32_t* const* groups, const int32_t* reps, int32_t n_groups, int32_t* roots,
                       double* root_ts, void* stream);

/* ------------------------------------------------------------------------------------------
 * BPR loss, forward + gradient in one pass (main.py:321-337 / 364-381):
 *   loss = -mean_b log sigmoid( mean_k( s_b.p_b - s_b.n_bk ) )       (sigma of the MEAN difference)
 * emb f32[R,D] holds the roots in the reference's order: [src B | dst B | (p_pos B*n_pos) | neg B*n_neg];
 * pos_off = row offset of the positives block (B for the baseline path where the positive is dst,
 * 2B for the `ours` path), neg_off = row offset of the negatives block.  n_pos must be 1 (main.py:33).
 * loss_out f32[1]; d_emb f32[R,D] receives scale * dloss/demb (rows not involved are zeroed).
 */
int pfo_bpr_loss(const float* emb, int64_t B, int32_t D, int64_t pos_off, int64_t neg_off, int32_t n_neg,
                 int64_t R, float scale, float* loss_out, float* d_emb, float* workspace, void* stream);
/* The same in ONE launch: the workgroup that finishes last takes the mean (index order: reproducible).  ticket i32[1]: zero
 * before the first use, resets itself; workspace f32[B]. */
int pfo_bpr_loss_fused(const float* emb, int64_t B, int32_t D, int64_t pos_off, int64_t neg_off, int32_t n_neg,
                       int64_t R, float scale, float* loss_out, float* d_emb, float* workspace, int32_t* ticket, void* stream);
/* Only the per-interaction losses loss_parts f32[B] (-log sigmoid of the mean score difference) and the gradient rows; the
 * mean over the batch is left to the caller (pfo_tgn_backward_ev takes it on its side stream). */
int pfo_bpr_loss_parts(const float* emb, int64_t B, int32_t D, int64_t pos_off, int64_t neg_off, int32_t n_neg,
                       int64_t R, float scale, float* loss_parts, float* d_emb, void* stream);

/* ------------------------------------------------------------------------------------------
 * Ranking metrics of evaluation.py:114-145 for one positive per interaction.
 *   emb f32[R,D] = [src B | dst B | neg B*n_items]; score = src . item (evaluation.py:114-115).
 *   rank_b = #{ k : score(neg_bk) >= score(dst_b) }  - position of the positive in the descending order of
 *   concat(pos, neg) with the canonical tie policy (stable ascending argsort reversed, SURVEY App. A-9;
 *   evaluation.py:138 uses the platform's unstable argsort).
 *   rank_out i32[B]; hits_out f32[B,3] = recall@{1,3,5}; ndcg_out f32[B,3] = NDCG@{1,3,5} (evaluation.py:11-21).
 */
int pfo_rank_metrics(const float* emb, int64_t B, int32_t D, int32_t n_items, int32_t* rank_out, float* hits_out,
                     float* ndcg_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * The whole per-interaction part of eval_recommendation (evaluation.py:114-207) in one launch: a superset of
 * pfo_rank_metrics that also ranks the head of the candidate list and evaluates the investment metrics.
 *   emb f32[B*(2+n_neg), D] = [src B | dst B | neg B*n_neg], 16-byte aligned, D a multiple of 4, D <= 256; read once.
 *   cand i32[B, 1+n_neg]: item node ids of the candidates, column 0 the destination (evaluation.py:176-178).
 *   day_idx i32[B]; port_idx i32[B, port_stride] stock indices, port_len i32[B] (0: the reference's `'' in portfolio`
 *   branch, evaluation.py:153-157); ret_past / ret_future f64[n_days, n_stocks, n_ret]: log-returns of
 *   time_feature_past / time_feature_future, np.log(p[1:] / p[:-1]) per stock (evaluation.py:31); a candidate's stock
 *   index is its node id - upper_u - 1.  A day or a stock outside the tables turns that row's figures into NaN.
 * Rows [out_row0, out_row0 + B) of buffers that hold out_rows rows are written (a whole evaluation pass accumulates in
 * one set of buffers and is read back once); any output pointer may be NULL:
 *   rank_out i32, hits_out f32[.,3], ndcg_out f32[.,3]: as pfo_rank_metrics.
 *   top5_pos i32[.,5]: positions into the 1+n_neg row of the five best candidates in the canonical order (stable
 *   ascending argsort reversed, SURVEY App. A-9: score descending, the larger position first among equal scores, so the
 *   positive comes last among its ties); top5_item i32[.,5]: their node ids; -1 where fewer than five candidates exist.
 *   invest_out f64[.,12] = (return@1,3,5 | sharpe@1,3,5) in-sample, then the same six out-of-sample: the change
 *   of mean(daily) * 251 and of mean(daily) * 251 / (std(daily, ddof=0) * sqrt(251)) when the top-k stocks' rows join the
 *   portfolio's (duplicates counted as often as they occur), daily = the mean log-return over the rows
 *   (return_sharpe_at_k, evaluation.py:23-36).  fp64 in numpy's order of operations; no guards (zero deviation: inf / nan).
 */
int pfo_eval_metrics(const float* emb, int64_t B, int32_t D, int32_t n_neg, const int32_t* cand, const int32_t* day_idx,
                     const int32_t* port_idx, const int32_t* port_len, int32_t port_stride, const double* ret_past,
                     const double* ret_future, int32_t n_days, int32_t n_stocks, int32_t n_ret, int32_t upper_u,
                     int64_t out_row0, int64_t out_rows, int32_t* rank_out, float* hits_out, float* ndcg_out,
                     int32_t* top5_pos, int32_t* top5_item, double* invest_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * pfo_eval_metrics with the row ranked in a SERVED order (abi 6, additive): the mean-variance rank fusion that
 * pfo_recommend_mv_topk serves (mode 0) or the basket rounds of pfo_recommend_basket_topk with k = 5 (mode 1), in one launch, one
 * workgroup per interaction.  The first 23 arguments are pfo_eval_metrics's, in its order and with its meaning; then
 *   ret_mv f64[mv_days, mv_stocks, mv_ret]: the table the ORDER is computed from (MVSampler.returns; it need not be ret_past or
 *   ret_future, and it numbers its own days: mv_day_idx i32[B]); gamma, lambda_mv; mode: 0 the fused list, 1 the basket;
 *   optional outputs, rows [out_row0, out_row0 + B) like the others: top5_fused f64[.,5], n_adm i32[.];
 *   optional diagnostics for the B rows of THIS call: score_out f32[B, 1+n_neg] (every candidate), y_out f64[B, 1+n_neg] and
 *   fused_out f64[B, 1+n_neg] (NaN outside A(b); in mode 1 fused_out is round 0's).
 * Score: score(b,c) is pfo_eval_metrics's to the bit (the same device function), not the matrix-core path of pfo_recommend_*.
 * Stock of candidate c: cand[b,c] - upper_u - 1.
 * Portfolio for y: the first min(port_len[b], port_stride) entries of port_idx[b] under pfo_recommend_mv_topk's rules - the
 *   length clamped to [0, port_stride], entries outside [0, mv_stocks) left out, duplicates kept, none left: the branch of
 *   main.py:254.  y(b,c) = y_mv of main.py:243-271 on ret_mv[mv_day_idx[b]] in fp64, numpy's order of operations, no
 *   contraction: the operations of pfo_recommend_mv_topk's y in its order.
 * Admissible set A(b): the candidates whose stock lies in [0, mv_stocks) and whose y is no NaN; +-inf are ordinary values.
 *   mv_day_idx[b] outside [0, mv_days): A(b) is empty and nothing of ret_mv is read.  n_adm = |A(b)|.
 * Mode 0: over A(b) the average-tie ranks (scipy rankdata) of y and of the fp32 score (-0 == +0),
 *   fused = lambda_mv * rank(y) + (1 - lambda_mv) * rank(score) (main.py:282-286); canonical order: fused descending, the LARGER
 *   position first among equal values.  top5_pos / top5_item / top5_fused: the first min(5, n_adm) of that order, the other slots
 *   -1 / -1 / -inf.  rank = the number of candidates in front of the positive (column 0) in that order.
 * Mode 1: rounds r = 0 .. 4 as pfo_recommend_basket_topk states them (steps 1-5, k = 5): the pick of round r is top5_pos[r],
 *   top5_fused[r] its fused value OF ROUND r (a row need not descend); only the picked position leaves the pool, the picked
 *   stock joins the holdings; a NaN y sits out its round only; the list ends when nobody takes part.  n_adm is round 0's |A(b)|.
 *   rank = the round in which the positive was picked.
 * The positive not ranked - it is not in A(b) (both modes), or no round picked it (mode 1): rank = PFO_EVAL_RANK_NONE, all three
 *   hits and NDCG values 0.  In mode 1 rank is therefore CENSORED at 5: it tells the place of a positive inside the basket and
 *   nothing about one outside it; recall / NDCG@{1,3,5} need no more.
 * hits_out / ndcg_out follow from rank as in pfo_eval_metrics.  invest_out: that function's investment stage - the same
 *   operations in the same order - fed with this top-5 and reading ret_past / ret_future by day_idx; a row with fewer than five
 *   picks adds what there is.
 * Bounds: 1 <= n_neg and 1 + n_neg <= PFO_RECOMMEND_MV_MAX_ITEMS (score, y, the three pieces of y and fused of a row live in
 *   LDS, 44 bytes per candidate, and the ranks are found by counting: about 3 (1+n_neg)^2 comparisons per row in mode 0, 10 in
 *   mode 1); 2 <= mv_ret <= 128; mode in {0, 1}; mv_days, mv_stocks > 0; everything pfo_eval_metrics checks.
 * Errors: all bounds are checked before any pointer is looked at (PFO_ERR_INVALID, nothing queued).  B == 0: PFO_OK.
 */
#define PFO_EVAL_RANK_NONE 2147483647
int pfo_eval_metrics_mv(const float* emb, int64_t B, int32_t D, int32_t n_neg, const int32_t* cand, const int32_t* day_idx,
                        const int32_t* port_idx, const int32_t* port_len, int32_t port_stride, const double* ret_past,
                        const double* ret_future, int32_t n_days, int32_t n_stocks, int32_t n_ret, int32_t upper_u,
                        int64_t out_row0, int64_t out_rows, int32_t* rank_out, float* hits_out, float* ndcg_out,
                        int32_t* top5_pos, int32_t* top5_item, double* invest_out, const double* ret_mv, int32_t mv_days,
                        int32_t mv_stocks, int32_t mv_ret, const int32_t* mv_day_idx, double gamma, double lambda_mv,
                        int32_t mode, double* top5_fused, int32_t* n_adm, float* score_out, double* y_out, double* fused_out,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * A served list scored against what happened (abi 6, additive): the place in the list of the item the user then took, and what
 * the first c stocks of the list would have done to the user's portfolio, at every cutoff c of a caller's choice - whatever
 * order produced the list (pfo_recommend_topk, _mv_topk, _mv_topk_wide, _basket_topk or anything else).  One launch, one
 * wavefront per user; nothing but the outputs is written.
 *   list_item i32[U, L]: item NODE ids, best first, 1 <= L <= 64.  n_valid i32[U] or NULL (= L everywhere), clamped to [0, L]:
 *   the slots in front of it count.  A slot holding a negative id is skipped; it ends nothing and keeps its place.
 *   truth i32[U]: the item the user took; < 0: none.
 *   cutoffs: a HOST array of n_c ints, 1 <= n_c <= 8, strictly increasing, each in [1, L].  Cutoff c = the first c SLOTS.
 *   port_idx i32[U, port_stride] stock indices, port_len i32[U] clamped to [0, port_stride] (both may be NULL with port_stride
 *   0); a list item's stock is its id - upper_u - 1; a stock that occurs twice - in the portfolio, in the list, or in both -
 *   counts twice.
 *   ret_past f64[past_days, past_stocks, n_ret] read at day_past i32[U], ret_future f64[future_days, future_stocks, n_ret] read
 *   at day_future i32[U]; 2 <= n_ret <= 128.  The two tables may be the same storage (a price ledger's, the days then ring
 *   slots).  A day outside a table turns THAT table's figures of the row into NaN; a stock outside a table those of that
 *   table from the first series it takes part in (a portfolio stock: all of them; the stock in slot t: the cutoffs > t).
 *   Nothing is read out of bounds, and the other table's figures are untouched (pfo_eval_metrics has one day index).
 * Rows [out_row0, out_row0 + U) of buffers that hold out_rows rows are written; any output pointer may be NULL:
 *   rank_out i32: the first counted slot that holds truth, else PFO_EVAL_RANK_NONE.
 *   hits_out f32[., n_c] = rank < c; ndcg_out f32[., n_c] = 1.f / log2f(rank + 2) where hit, else 0: pfo_eval_metrics's
 *   expression, bit-equal to its values at the ranks it can state (< 5).  log2f is the device library's (1 ulp): the value lies
 *   within 3 ulp of the correctly rounded 1 / log2(rank + 2) and is exact where rank + 2 is a power of two.
 *   invest_out f64[., 4 n_c] = (return@c.. | sharpe@c..) in-sample, then the same out-of-sample: pfo_eval_metrics's investment
 *   stage at the cutoffs - per table the per-day sum over the portfolio rows, then the list's rows added one at a time, divided
 *   by the row count at each cutoff (a list shorter than a cutoff adds what there is); mean and population deviation in numpy's
 *   summation order; return = mean * 251, sharpe = return / (sd * sqrt(251)); an empty portfolio alone is 0, 0; no guards.
 *   fp64, no contraction: with cutoffs (1, 3, 5) on pfo_eval_metrics's top5_item this is its invest_out to the bit.
 * Errors: all bounds are checked before any device pointer is looked at (PFO_ERR_INVALID, nothing queued).  U == 0: PFO_OK.
 */
int pfo_list_metrics(const int32_t* list_item, const int32_t* n_valid, const int32_t* truth, int64_t U, int32_t L,
                     const int32_t* cutoffs, int32_t n_c, const int32_t* port_idx, const int32_t* port_len, int32_t port_stride,
                     int32_t upper_u, const double* ret_past, const int32_t* day_past, int32_t past_days, int32_t past_stocks,
                     const double* ret_future, const int32_t* day_future, int32_t future_days, int32_t future_stocks,
                     int32_t n_ret, int64_t out_row0, int64_t out_rows, int32_t* rank_out, float* hits_out, float* ndcg_out,
                     double* invest_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Read-only top-k recommendation: scores a tile of users against ONE shared candidate matrix and keeps the k best per user
 * (one launch; the U x I score matrix never reaches memory).
 *   user_emb f32[U,D]; item_emb f32[n_t*I, D]: n_t blocks of the same I candidates embedded at n_t times;
 *   user_block i32[U] in [0,n_t) (NULL: all 0): the block user u is scored against (a value outside the range is clamped
 *   into it).  Both matrices 16-byte aligned.
 *   score(u,i) = user_emb[u] . item_emb[user_block[u]*I + i] in fp32 on the fp32 matrix core (v_mfma_f32_16x16x4_f32: exact
 *   products, fp32 accumulation - within the fp32 dot-product error bound, NOT the split 16-bit contraction).
 *   Candidate i is skipped for user u when item_ok != NULL && item_ok[i] == 0, or when i occurs in
 *   excl_pos[u, 0:excl_len[u]] (candidate POSITIONS, rows of excl_stride entries; entries < 0 or >= I are ignored, duplicates
 *   allowed, excl_len is clamped to [0, excl_stride]).
 *   Order: score descending; among equal scores (-0 == +0) the LARGER position first - the canonical order of
 *   SURVEY App. A-9 that pfo_eval_metrics uses.  A NaN score is outside the contract.
 *   top_pos i32[U,k], top_score f32[U,k] (a zero score is returned as +0); slots beyond the number of admissible candidates
 *   hold -1 / -inf; n_valid i32[U] (optional) = min(k, #admissible).
 *   D % 4 == 0, D <= 256, 1 <= k <= 64, 1 <= I <= PFO_RECOMMEND_MAX_ITEMS.  The candidates pass through LDS 512 at a time with
 *   the best k so far carried along, so LDS bounds nothing; the constant bounds the time of one workgroup.
 */
#define PFO_RECOMMEND_MAX_ITEMS 65536
int pfo_recommend_topk(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U, int32_t I,
                       int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len, int32_t excl_stride,
                       const uint8_t* item_ok, int32_t k, int32_t* top_pos, float* top_score, int32_t* n_valid, void* stream);

/* ------------------------------------------------------------------------------------------
 * Portfolio-aware top-k: pfo_recommend_topk with the mean-variance rank fusion of main.py:243-289 applied to the whole candidate
 * list of every user, in one launch; nothing of size U x I reaches memory unless a diagnostic array is asked for.
 *   The first eleven arguments are pfo_recommend_topk's, and score(u,i) is its score to the bit (same matrix-core path, same
 *   accumulation order).
 *   cand_stock i32[I]: row of candidate i in `returns`; returns f64[n_days, n_stocks, n_ret]: log-returns, np.log(p[1:] / p[:-1])
 *   per stock (MVSampler.returns); day_idx i32[U]; port_idx i32[U, port_stride], port_len i32[U] (clamped to [0, port_stride]):
 *   the portfolio of u is the entries in [0, n_stocks) among the first port_len[u], duplicates counted as often as they occur;
 *   none left (or port_idx NULL): the empty-portfolio branch, main.py:254.
 *   y(u,i) = y_mv of main.py:243-271 in fp64, numpy's order of operations, no contraction - the arithmetic of pfo_mv_select
 *   (from eight holdings on, np.sum adds the covariances pairwise and the last bits may differ from this sequential sum).
 *   Admissible set A(u): the rules of pfo_recommend_topk (item_ok, excl_pos), minus candidates with cand_stock outside
 *   [0, n_stocks), minus candidates whose y is NaN (a constant price series: 0 / 0); +-inf are ordinary values.  A user whose
 *   day_idx is outside [0, n_days) has an empty A(u) and nothing is read for it.
 *   Over A(u) alone, n = |A(u)|: invest_rank = average-tie rank of y (scipy rankdata, main.py:282); tgn_rank = average-tie rank
 *   of the fp32 score, -0 == +0 (it stands in for the positional n..1 of main.py:283, "the model's order");
 *   fused = lambda_mv * invest_rank + (1 - lambda_mv) * tgn_rank (main.py:286).
 *   Order: stable ascending argsort of fused, reversed: fused descending, the LARGER position first among equal
 *   values.  top_pos i32[U,k], top_score f32[U,k] (a zero score as +0), top_fused f64[U,k]: the first min(k, n) of that order,
 *   the other slots -1 / -inf / -inf; n_valid i32[U] (optional) = min(k, n).
 *   Diagnostics, each optional: score_out f32[U,I] (every i), y_out / fused_out f64[U,I] (NaN outside A(u)).
 *   D % 4 == 0, D <= 256, 1 <= k <= 64, 1 <= I <= PFO_RECOMMEND_MV_MAX_ITEMS (scores, y and ranks of a user live in LDS),
 *   2 <= n_ret <= 128, 1 <= n_t.
 */
#define PFO_RECOMMEND_MV_MAX_ITEMS 2048
int pfo_recommend_mv_topk(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U, int32_t I,
                          int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len, int32_t excl_stride,
                          const uint8_t* item_ok, const int32_t* cand_stock, const double* returns, int32_t n_days,
                          int32_t n_stocks, int32_t n_ret, const int32_t* day_idx, const int32_t* port_idx,
                          const int32_t* port_len, int32_t port_stride, double gamma, double lambda_mv, int32_t k,
                          int32_t* top_pos, float* top_score, double* top_fused, int32_t* n_valid, float* score_out,
                          double* y_out, double* fused_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * The wide form of the portfolio-aware top-k (abi 6, additive): pfo_recommend_mv_topk for candidate lists LDS cannot hold.
 *   The first 30 arguments are pfo_recommend_mv_topk's and the contract is that function's, word for word - scores, A(u), the
 *   portfolio rules, the y arithmetic, average-tie ranks (-0 == +0 for both keys, +-inf ordinary values, a NaN y outside A(u)),
 *   blend, canonical order, empty slots, n_valid, a zero score as +0, the three optional diagnostic arrays - with ONE difference:
 *   1 <= I <= PFO_RECOMMEND_MV_WIDE_MAX_ITEMS.  For I <= PFO_RECOMMEND_MV_MAX_ITEMS every output equals pfo_recommend_mv_topk's
 *   bit for bit: scores, y, ranks and blend come from the same device functions, and a rank is an exact (half-)integer however
 *   it is found.
 *   The state of a user lives in `workspace` (device memory, 16-byte aligned), and the ranks are found by sorting: per user an
 *   LSD radix sort of the admissible candidates' y keys (8 passes) and score keys (4 passes), two binary searches per candidate
 *   and key, k reads of the fused row for the selection - O(I log I) per user, nothing counts pairs.
 *   Workspace layout: with IP = I rounded up to 16 and R = 16 * (tiles of the slab) user rows, six arrays one after another:
 *     y / fused f64[R, IP] (8 bytes per user and candidate), y keys u64[R, IP] twice (8 + 8), score f32[R, IP] (4),
 *     score keys u32[R, IP] twice (4 + 4): 36 bytes per user and candidate.
 *   pfo_recommend_mv_wide_workspace_bytes(U, I) = 36 * 16 * ceil(U / 16) * IP (host arithmetic, no device; U < 1 and I < 1 count
 *   as 1) serves all U users in one slab.  The entry accepts any workspace_bytes >= ..._bytes(min(U, 16), I) and serves the users in
 *   slabs of as many 16-user tiles as fit, queued in order on `stream` (two launches per slab, whatever the data); the result
 *   does not depend on the slab size.  No allocation, no host synchronisation, no read-back.
 *   Errors (PFO_ERR_INVALID, nothing queued): those of pfo_recommend_mv_topk; I outside the bound above; with U > 0 a null,
 *   short or misaligned workspace.  U == 0: PFO_OK, no pointer is looked at.
 */
#define PFO_RECOMMEND_MV_WIDE_MAX_ITEMS PFO_RECOMMEND_MAX_ITEMS
int64_t pfo_recommend_mv_wide_workspace_bytes(int64_t U, int32_t I);
int pfo_recommend_mv_topk_wide(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U, int32_t I,
                               int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len, int32_t excl_stride,
                               const uint8_t* item_ok, const int32_t* cand_stock, const double* returns, int32_t n_days,
                               int32_t n_stocks, int32_t n_ret, const int32_t* day_idx, const int32_t* port_idx,
                               const int32_t* port_len, int32_t port_stride, double gamma, double lambda_mv, int32_t k,
                               int32_t* top_pos, float* top_score, double* top_fused, int32_t* n_valid, float* score_out,
                               double* y_out, double* fused_out, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Basket top-k (abi 6, additive): the list of pfo_recommend_mv_topk taken one pick at a time, each pick joining the holdings
 * before the next is ranked, in one launch.  The arguments are pfo_recommend_mv_topk's without the three diagnostic arrays and
 * mean what they mean there: scores, admissible set A(u), portfolio P (list order, out-of-range entries left out, duplicates
 * kept), y_mv arithmetic, average-tie ranks, blend and canonical order are that function's.
 *   For round r = 0 .. k-1 of user u:
 *     1. P_r = P followed by cand_stock[pick_0 .. pick_{r-1}] in pick order.  y_r[c] = y_mv of candidate c against P_r - fp64,
 *        no contraction, the covariances summed in that order - for every c of A(u) that has not been picked.  A candidate
 *        whose y_r is NaN sits out round r only.
 *     2. invest_rank / tgn_rank: the average-tie ranks of y_r and of the fp32 score over the candidates taking part in round r;
 *        fused_r = lambda_mv * invest_rank + (1 - lambda_mv) * tgn_rank.
 *     3. pick_r = the first of the canonical order: fused_r descending, the LARGER position first among equal values.
 *     4. top_pos[u,r] = pick_r, top_score[u,r] = its score (a zero as +0), top_fused[u,r] = fused_r[pick_r] - the value of
 *        round r, so top_fused need not descend along a row.
 *     5. Nobody takes part: the list ends; n_valid[u] (optional) = number of picks, the other slots hold -1 / -inf / -inf.
 *   Only the picked POSITION leaves the pool: another candidate on the same stock stays (and now carries the covariance with
 *   itself).  The picked stock joins P_r even if it is held already.  A user whose day_idx is outside [0, n_days) gets an
 *   empty list.
 *   Hence: k = 1 is pfo_recommend_mv_topk(k = 1) bit for bit; lambda_mv = 0 gives pfo_recommend_mv_topk's positions for any k;
 *   any k equals k calls of pfo_recommend_mv_topk(k = 1) with each pick appended to the portfolio row and the exclusion row.
 *   Bounds as for pfo_recommend_mv_topk.  Work per user: 2 k I^2 comparisons, (|P| + k - 1) I n_ret multiply-adds.
 */
int pfo_recommend_basket_topk(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U, int32_t I,
                              int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len, int32_t excl_stride,
                              const uint8_t* item_ok, const int32_t* cand_stock, const double* returns, int32_t n_days,
                              int32_t n_stocks, int32_t n_ret, const int32_t* day_idx, const int32_t* port_idx,
                              const int32_t* port_len, int32_t port_stride, double gamma, double lambda_mv, int32_t k,
                              int32_t* top_pos, float* top_score, double* top_fused, int32_t* n_valid, void* stream);

/* ------------------------------------------------------------------------------------------
 * Group caps (abi 6, additive): the three entries above with a concentration limit - at most group_cap picks of a group (a
 * sector, an exchange, an issuer, a risk bucket) in a user's list - in the same one launch.  Each takes its sibling's parameter
 * list with two arguments behind item_ok:
 *   cand_group i32[I], aligned with the candidates: the group of candidate c, any non-negative int32 (the kernels compare ids:
 *   no table by group, no bound on the number of groups); cand_group[c] < 0: c is in no group and is never capped.
 *   group_cap >= 1.
 * pfo_recommend_topk_capped / pfo_recommend_mv_topk_capped: the admissible set, the scores, y, the two average-tie ranks (counted
 *   over the WHOLE admissible set: a cap changes no rank), the blend and the canonical order are the sibling's.  The list is the
 *   walk over that order that takes a candidate unless its group is >= 0 and holds group_cap picks already, and stops at k.
 *   top_score / top_fused: the uncapped values of the picks.  n_valid = the number taken = min(k, #groupless admissible +
 *   sum over groups of min(group_cap, #admissible of the group)); the other slots -1 / -inf / -inf.  The diagnostics of the
 *   mean-variance form (score_out, y_out, fused_out) hold the uncapped values of every admissible candidate.
 *   Equivalently: a candidate survives iff fewer than group_cap admissible candidates of its group stand before it in the
 *   canonical order, and the list is the first k survivors.
 * pfo_recommend_basket_topk_capped: the pool of round r is A(u) minus the picks minus every candidate of a group that holds
 *   group_cap picks; a candidate outside the pool takes part in no rank count of the round, exactly like an excluded one.  The
 *   rest of a round is pfo_recommend_basket_topk's.  Hence: any k equals k calls of pfo_recommend_mv_topk(k = 1) with each pick
 *   appended to the portfolio row and the exclusion row and, once the pick's group is full, every other candidate of that group
 *   appended to the exclusion row as well.
 * With group_cap >= k, with every cand_group < 0, or with every candidate in a group of its own, every output is the sibling's
 * bit for bit.  There is no capped wide form and no capped list form.
 * Bounds and errors: the sibling's, plus group_cap < 1 (checked with the bounds) and, with U > 0, a null cand_group.  U == 0:
 * PFO_OK, no pointer is looked at.  Work on top of the sibling's: a few wave-wide operations per round (plain), one pass of
 * I^2 comparisons per user (mean-variance), at most k LDS reads per pick (basket); 4 bytes of LDS per candidate held.
 */
int pfo_recommend_topk_capped(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U, int32_t I,
                              int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len, int32_t excl_stride,
                              const uint8_t* item_ok, const int32_t* cand_group, int32_t group_cap, int32_t k, int32_t* top_pos,
                              float* top_score, int32_t* n_valid, void* stream);
int pfo_recommend_mv_topk_capped(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U, int32_t I,
                                 int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len, int32_t excl_stride,
                                 const uint8_t* item_ok, const int32_t* cand_group, int32_t group_cap, const int32_t* cand_stock,
                                 const double* returns, int32_t n_days, int32_t n_stocks, int32_t n_ret, const int32_t* day_idx,
                                 const int32_t* port_idx, const int32_t* port_len, int32_t port_stride, double gamma,
                                 double lambda_mv, int32_t k, int32_t* top_pos, float* top_score, double* top_fused,
                                 int32_t* n_valid, float* score_out, double* y_out, double* fused_out, void* stream);
int pfo_recommend_basket_topk_capped(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U, int32_t I,
                                     int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len, int32_t excl_stride,
                                     const uint8_t* item_ok, const int32_t* cand_group, int32_t group_cap,
                                     const int32_t* cand_stock, const double* returns, int32_t n_days, int32_t n_stocks,
                                     int32_t n_ret, const int32_t* day_idx, const int32_t* port_idx, const int32_t* port_len,
                                     int32_t port_stride, double gamma, double lambda_mv, int32_t k, int32_t* top_pos,
                                     float* top_score, double* top_fused, int32_t* n_valid, void* stream);

/* ------------------------------------------------------------------------------------------
 * Group caps that count holdings (abi 6, additive): the three capped entries with a per-user starting count - what a user
 * already holds of a group uses up that much of the group's quota.  Each takes its _capped sibling's parameter list with three
 * arguments directly behind group_cap:
 *   held_group i32[U, held_stride], padded with -1: one group id per holding of user u;  held_len i32[U], clamped to
 *   [0, held_stride];  0 <= held_stride <= PFO_RECOMMEND_HELD_MAX_WIDTH.
 *   h_u(g) = the number of entries p < held_len[u] with held_group[u, p] == g.  A negative entry is a holding in no group and
 *   counts for nothing; an id named twice counts twice.
 * pfo_recommend_topk_capped_held / pfo_recommend_mv_topk_capped_held: the walk of the sibling takes a candidate of group g >= 0
 *   unless (picks of g so far) + h_u(g) >= group_cap; a group with h_u(g) >= group_cap is closed from the start.  The
 *   admissible set, ranks (over the WHOLE admissible set), values and diagnostics are the uncapped ones.  Equivalently: a
 *   candidate survives iff (admissible candidates of its group before it in the canonical order) + h_u(g) < group_cap.
 * pfo_recommend_basket_topk_capped_held: the pool of round r is A(u) minus the picks minus every candidate of a group with
 *   picks + h_u(g) >= group_cap - in round 0 too, so a group closed from the start takes part in no rank count, exactly like
 *   excluded candidates.
 * n_valid = min(k, #groupless admissible + sum over groups of min(max(group_cap - h_u(g), 0), #admissible of the group)).
 * With every held_len 0, or held_stride 0 (the two pointers may then be null), every output is the _capped sibling's bit for bit.
 * Bounds and errors: the sibling's, plus held_stride outside [0, PFO_RECOMMEND_HELD_MAX_WIDTH] (checked with the bounds) and,
 * with U > 0 and held_stride > 0, a null held_group or held_len.  LDS on top of the sibling's: 4 held_stride bytes (mean-variance,
 * basket: the row of the user being served), 128 held_stride + 128 bytes (plain: the rows of a tile's 16 users, twice, and
 * their lengths).
 */
#define PFO_RECOMMEND_HELD_MAX_WIDTH 256
int pfo_recommend_topk_capped_held(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U, int32_t I,
                                   int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len, int32_t excl_stride,
                                   const uint8_t* item_ok, const int32_t* cand_group, int32_t group_cap, const int32_t* held_group,
                                   const int32_t* held_len, int32_t held_stride, int32_t k, int32_t* top_pos, float* top_score,
                                   int32_t* n_valid, void* stream);
int pfo_recommend_mv_topk_capped_held(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U, int32_t I,
                                      int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len, int32_t excl_stride,
                                      const uint8_t* item_ok, const int32_t* cand_group, int32_t group_cap, const int32_t* held_group,
                                      const int32_t* held_len, int32_t held_stride, const int32_t* cand_stock, const double* returns,
                                      int32_t n_days, int32_t n_stocks, int32_t n_ret, const int32_t* day_idx, const int32_t* port_idx,
                                      const int32_t* port_len, int32_t port_stride, double gamma, double lambda_mv, int32_t k,
                                      int32_t* top_pos, float* top_score, double* top_fused, int32_t* n_valid, float* score_out,
                                      double* y_out, double* fused_out, void* stream);
int pfo_recommend_basket_topk_capped_held(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U, int32_t I,
                                          int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len, int32_t excl_stride,
                                          const uint8_t* item_ok, const int32_t* cand_group, int32_t group_cap,
                                          const int32_t* held_group, const int32_t* held_len, int32_t held_stride,
                                          const int32_t* cand_stock, const double* returns, int32_t n_days, int32_t n_stocks,
                                          int32_t n_ret, const int32_t* day_idx, const int32_t* port_idx, const int32_t* port_len,
                                          int32_t port_stride, double gamma, double lambda_mv, int32_t k, int32_t* top_pos,
                                          float* top_score, double* top_fused, int32_t* n_valid, void* stream);

/* ------------------------------------------------------------------------------------------
 * The list form of the two top-k entries (abi 6, additive): every user ranks a list of its OWN, not the shared candidate list
 * minus an exclusion list.  user_emb, item_emb, user_block, U, I, n_t, D, item_ok, k and the mean-variance arguments mean what
 * they mean in pfo_recommend_topk / pfo_recommend_mv_topk; the exclusion triple gives way to
 *   list_pos i32[U, list_stride], list_len i32[U]: candidate POSITIONS into the I candidates of a block.
 *   Admissible set A(u): the DISTINCT positions p among the first min(max(list_len[u], 0), list_stride) entries of row u with
 *   0 <= p < I and (item_ok == NULL || item_ok[p] != 0); in the mean-variance form also with a y (day and cand_stock inside the
 *   tables, y not NaN: pfo_recommend_mv_topk's rule).  Entries outside [0, I) are ignored (the -1 padding, a holding that is
 *   not among the candidates); a position named more than once counts once, for the selection and for both ranks; an empty list
 *   gives an empty answer.
 *   score(u, p) = user_emb[u] . item_emb[user_block[u]*I + p] in fp32 - four partial sums per lane, then across four lanes, NOT
 *   the matrix-core order of pfo_recommend_topk: a score is within the any-order fp32 dot-product bound of the exact value and
 *   equals pfo_recommend_topk's only where both are exact.  The two list entries compute the same score to the bit.
 *   Order, -0 == +0, empty slots (-1 / -inf / -inf), n_valid = min(k, |A(u)|), a zero score as +0, y (pfo_recommend_mv_topk's
 *   arithmetic), the average-tie ranks over A(u) and the blend: as in pfo_recommend_topk / pfo_recommend_mv_topk.  The portfolio
 *   is used as given: a list of a user's own holdings is ranked against those holdings, itself among them.
 *   Diagnostics, each optional, BY LIST SLOT: score_out f32[U, list_stride], y_out / fused_out f64[U, list_stride]; NaN in every
 *   slot that is not the first occurrence of an admissible position.
 *   Bounds, all checked before any pointer is looked at (PFO_ERR_INVALID, nothing queued): D % 4 == 0, D <= 256, 1 <= k <= 64,
 *   1 <= I <= PFO_RECOMMEND_MAX_ITEMS (no 2048 here: only the list is ranked), 1 <= n_t,
 *   1 <= list_stride <= PFO_RECOMMEND_LIST_MAX_WIDTH, 2 <= n_ret <= 128, port_stride >= 0.  U == 0: PFO_OK, no pointer is
 *   looked at.  One launch, one wavefront per user; the users need not be sorted by block.  W D multiply-adds and about 3 W^2
 *   comparisons (mean-variance form) per user, W = the list's length.
 */
#define PFO_RECOMMEND_LIST_MAX_WIDTH 256
int pfo_recommend_list_topk(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U, int32_t I,
                            int32_t n_t, int32_t D, const int32_t* list_pos, const int32_t* list_len, int32_t list_stride,
                            const uint8_t* item_ok, int32_t k, int32_t* top_pos, float* top_score, int32_t* n_valid,
                            float* score_out, void* stream);
int pfo_recommend_list_mv_topk(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U, int32_t I,
                               int32_t n_t, int32_t D, const int32_t* list_pos, const int32_t* list_len, int32_t list_stride,
                               const uint8_t* item_ok, const int32_t* cand_stock, const double* returns, int32_t n_days,
                               int32_t n_stocks, int32_t n_ret, const int32_t* day_idx, const int32_t* port_idx,
                               const int32_t* port_len, int32_t port_stride, double gamma, double lambda_mv, int32_t k,
                               int32_t* top_pos, float* top_score, double* top_fused, int32_t* n_valid, float* score_out,
                               double* y_out, double* fused_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Position-weighted mean-variance order (abi 6, additive): the three entries that compute y from a portfolio and serve a list,
 * with a weight per holding in place of 1 / n_holding.  Each takes its sibling's parameter list with port_w f64[U, port_stride]
 * (row stride port_stride, aligned with port_idx) behind port_len.
 *   Holding p of user u counts iff port_idx[u, p] is in [0, n_stocks) AND port_w[u, p] is finite and > 0 - a zero, negative, NaN
 *   or infinite weight leaves the holding out exactly as an out-of-range stock is left out.  Over the counted holdings in row
 *   order, fp64, every product rounded before it is added: ssum_w = sequential sum of port_w[u, p] * cov(i, p) (the covariance as
 *   in pfo_recommend_mv_topk, one rounded product, one rounded add), wsum = sequential sum of port_w[u, p],
 *   y = (mu / gamma - 0.5 * ((1.0 / wsum) * ssum_w)) / var; no counted holding: y = (mu / gamma) / var.
 *   With every weight exactly 1.0 that is the sibling's y bit for bit; scaling a user's weights by a power of two changes no bit.
 *   Everything else - scores, admissible set, ranks, blend, canonical order, empty slots, diagnostics - is the sibling's.
 *   port_w == NULL forwards to the sibling, bit for bit.  port_w without port_idx (port_stride > 0, U > 0) is PFO_ERR_INVALID,
 *   checked where port_idx without port_len is.  Bounds, error order and U == 0 behaviour are the sibling's.
 *   There is no weighted basket and no weighted capped form.
 */
int pfo_recommend_mv_topk_weighted(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U, int32_t I,
                                   int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len, int32_t excl_stride,
                                   const uint8_t* item_ok, const int32_t* cand_stock, const double* returns, int32_t n_days,
                                   int32_t n_stocks, int32_t n_ret, const int32_t* day_idx, const int32_t* port_idx,
                                   const int32_t* port_len, const double* port_w, int32_t port_stride, double gamma, double lambda_mv,
                                   int32_t k, int32_t* top_pos, float* top_score, double* top_fused, int32_t* n_valid, float* score_out,
                                   double* y_out, double* fused_out, void* stream);
int pfo_recommend_mv_topk_wide_weighted(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U, int32_t I,
                                        int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len, int32_t excl_stride,
                                        const uint8_t* item_ok, const int32_t* cand_stock, const double* returns, int32_t n_days,
                                        int32_t n_stocks, int32_t n_ret, const int32_t* day_idx, const int32_t* port_idx,
                                        const int32_t* port_len, const double* port_w, int32_t port_stride, double gamma,
                                        double lambda_mv, int32_t k, int32_t* top_pos, float* top_score, double* top_fused,
                                        int32_t* n_valid, float* score_out, double* y_out, double* fused_out, void* workspace,
                                        int64_t workspace_bytes, void* stream);
int pfo_recommend_list_mv_topk_weighted(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U, int32_t I,
                                        int32_t n_t, int32_t D, const int32_t* list_pos, const int32_t* list_len, int32_t list_stride,
                                        const uint8_t* item_ok, const int32_t* cand_stock, const double* returns, int32_t n_days,
                                        int32_t n_stocks, int32_t n_ret, const int32_t* day_idx, const int32_t* port_idx,
                                        const int32_t* port_len, const double* port_w, int32_t port_stride, double gamma,
                                        double lambda_mv, int32_t k, int32_t* top_pos, float* top_score, double* top_fused,
                                        int32_t* n_valid, float* score_out, double* y_out, double* fused_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Time-sorted adjacency built on the device: replaces get_neighbor_finder / NeighborFinder.__init__ (utils/utils.py:117-148).
 * Every edge e contributes (dst, eidx, ts) to row src[e] and (src, eidx, ts) to row dst[e]; rows are sorted by timestamp,
 * ties in edge order (Python's stable sorted(key=ts), utils.py:139).  A stable LSD radix sort of the 2E entries; the eight
 * timestamp passes are skipped when the log is already chronological.  All pointers are device pointers; `workspace` holds
 * pfo_csr_build_workspace_bytes(E, n_nodes) bytes; indptr has n_nodes + 1 entries, the adjacency arrays 2E.
 * -0.0 and +0.0 are ONE timestamp to the sort (a tie, kept in edge order); adj_ts keeps the bits it was given.  NaN timestamps
 * have no place in the order: the Python callers refuse them, this entry does not look.
 */
int64_t pfo_csr_build_workspace_bytes(int64_t E, int64_t n_nodes);
int pfo_csr_build(const int32_t* src, const int32_t* dst, const int32_t* eidx, const double* ts, int64_t E, int64_t n_nodes,
                  int64_t* indptr, int32_t* adj_nbr, int32_t* adj_eidx, double* adj_ts, void* workspace,
                  int64_t workspace_bytes, void* stream);
/* What pfo_csr_build would launch for these sizes, asked without launching (pure host code; additive: the abi version stays):
 * out[0] = 1024-entry tiles of a radix pass, out[1] = owner passes (one per byte of the largest node id), out[2] = sweeps of
 * the scan over the 256 * tiles tile histograms (pfo_debug_scan_sweeps).  -1 with a message on sizes pfo_csr_build refuses. */
int pfo_debug_csr_build_plan(int64_t E, int64_t n_nodes, int32_t* out /* HOST, 3 entries */);
/* Merge of a CSR of NEW edges (built by pfo_csr_build over n_nodes rows) into an existing one (n_old_nodes <= n_nodes rows):
 * the result equals a rebuild over [old edges ; new edges] - inside a row a new entry goes behind every old entry whose
 * timestamp is <= its own.  Output arrays hold old + new entries; new_indptr has n_nodes + 1 entries.
 */
int pfo_csr_append(const int64_t* old_indptr, const int32_t* old_nbr, const int32_t* old_eidx, const double* old_ts,
                   int64_t n_old_nodes, const int64_t* add_indptr, const int32_t* add_nbr, const int32_t* add_eidx,
                   const double* add_ts, int64_t n_nodes, int64_t* new_indptr, int32_t* new_nbr, int32_t* new_eidx,
                   double* new_ts, void* stream);
/* Retention (abi 6, additive): every entry with ts < cutoff leaves the adjacency - strict, compared in fp64 on the stored fp64
 * timestamps.  Rows are time-sorted, so row v keeps the suffix [first_kept[v], indptr[v + 1]); n_nodes is unchanged, rows may
 * become empty.  The result equals masking the flat arrays with ts >= cutoff and re-accumulating indptr, bit for bit.
 *   pfo_csr_expire_plan : per-row lower bound -> first_kept i64[n_nodes], kept counts, exclusive scan -> new_indptr
 *                         i64[n_nodes + 1] (new_indptr[n_nodes] = the surviving total, which the caller reads back to size the
 *                         output).  Two launches; scratch holds pfo_csr_expire_scratch_bytes(n_nodes) bytes.  ts may be NULL
 *                         when the adjacency has no entries.
 *   pfo_csr_expire_copy : the surviving suffixes into new arrays of `total` entries (total = new_indptr[n_nodes]); one launch,
 *                         one lane per surviving entry.  total == 0 queues nothing.
 * PFO_ERR_INVALID - nothing is queued: n_nodes < 1, a cutoff that is NaN or infinite, a null pointer, a short scratch.
 */
int64_t pfo_csr_expire_scratch_bytes(int64_t n_nodes);
int pfo_csr_expire_plan(const int64_t* indptr, const double* ts, int64_t n_nodes, double cutoff, int64_t* first_kept,
                        int64_t* new_indptr, void* scratch, int64_t scratch_bytes, void* stream);
int pfo_csr_expire_copy(const int64_t* old_indptr, const int32_t* old_nbr, const int32_t* old_eidx, const double* old_ts,
                        int64_t n_nodes, const int64_t* first_kept, const int64_t* new_indptr, int64_t total, int32_t* new_nbr,
                        int32_t* new_eidx, double* new_ts, void* stream);

/* ------------------------------------------------------------------------------------------
 * Adam step over a flat parameter buffer (torch.optim.Adam defaults, main.py:123,389).
 */
int pfo_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                  float beta1, float beta2, float eps, int32_t step, void* stream);
/* The same update on up to PFO_ADAM_MAX_RANGES element ranges [lo[r], hi[r]) of the flat buffers, each with its own step
 * count, in ONE launch.  torch.optim.Adam keeps a step counter per parameter tensor and skips tensors whose .grad is
 * None (main.py:123 hands it every parameter; the GRU's are None on the first batch of an epoch, when no message is
 * pending: memory_updater.py:38-40), so tensors can be one step apart for a whole run; ranges that are left out are
 * not touched at all.  lo / hi / step are HOST arrays. */
/* ..._dev: the step count of range r is step[r] + *step_dev (a device word): a graph-captured step advances it on the device
 * and the bias corrections are computed there */
#define PFO_ADAM_MAX_RANGES 16
int pfo_adam_step_ranges_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int32_t n_ranges,
                             const int64_t* lo, const int64_t* hi, const int32_t* step, const int32_t* step_dev, float lr,
                             float beta1, float beta2, float eps, void* stream);
int pfo_adam_step_ranges(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int32_t n_ranges,
                         const int64_t* lo, const int64_t* hi, const int32_t* step, float lr, float beta1, float beta2,
                         float eps, void* stream);

/* What goes in FRONT of the Adam launch when FusedAdam clips or decays (csrc/optim.hip): global-norm clipping after
 * torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2) and the decoupled weight decay of torch.optim.AdamW, over
 * the same (n_ranges <= PFO_ADAM_MAX_RANGES, lo[], hi[]) description of the flat buffers (HOST arrays, arbitrary element
 * offsets, lo[r] == hi[r] allowed).  Both queue on `stream` and never synchronise with the host.
 *   pfo_grad_sumsq_ranges   : partial[PFO_GRAD_NORM_PARTS] (f64, device) = / += the sum of squares of the listed elements of
 *                             grad, one slot per workgroup.  Which element feeds which slot, and in which order, is a function
 *                             of (lo, hi, PFO_GRAD_NORM_PARTS) alone - no float atomics, no dependence on timing: two runs give
 *                             the same bits.  accumulate = 0 overwrites EVERY slot, 1 adds to it (a step of more than
 *                             PFO_ADAM_MAX_RANGES ranges: chunks in stream order).
 *   pfo_grad_prestep_ranges : every workgroup folds partial in index order (the same bits everywhere), total = (float)sqrt(sum),
 *                             coef = max_norm / (total + 1e-6f) clamped to at most 1 (fp32; a NaN stays a NaN), then
 *                             grad[i] *= coef and param[i] *= decay over the ranges; workgroup 0 stores total to norm_out (f32[1]).
 *                             max_norm <= 0: no clipping - partial and norm_out may be NULL, grad is not written.
 *                             decay == 1: param is not written.  Elements outside the ranges are never touched.
 * PFO_ERR_INVALID - nothing is queued: a NULL pointer that is needed, n_ranges outside [1, PFO_ADAM_MAX_RANGES], lo > hi, lo < 0. */
#define PFO_GRAD_NORM_PARTS 256
int pfo_grad_sumsq_ranges(const float* grad, int32_t n_ranges, const int64_t* lo, const int64_t* hi, double* partial,
                          int32_t accumulate, void* stream);
int pfo_grad_prestep_ranges(float* param, float* grad, int32_t n_ranges, const int64_t* lo, const int64_t* hi,
                            const double* partial, float max_norm, float decay, float* norm_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * The TGN step (model/tgn.py:102-378 + modules/).  One POD config, one flat parameter buffer,
 * caller-owned state tables and workspace.
 */
typedef struct pfo_tgn_config {
  int32_t n_nodes;      /* incl. padding node 0 */
  int32_t n_edges_p1;   /* rows of edge_feat (E+1) */
  int32_t D;            /* memory = node-feature = time dim (tgn.py:43-54); must be a multiple of 4 */
  int32_t Ef;           /* edge-feature dim (multiple of 4) */
  int32_t n_layers;     /* L */
  int32_t n_heads;      /* H, divides 2D */
  int32_t use_memory;   /* 0 = TGAT (main.py:70-74) */
  int32_t max_roots;    /* capacity R the workspace is sized for */
  int32_t max_neighbors;/* capacity K */
  int32_t max_batch;    /* capacity B (positives = 2B) */
  /* message function (modules/message_function.py): msg_dim == 0 = identity (the GRU reads the raw message, 3D+Ef wide);
     msg_dim > 0 = the MLP Linear(3D+Ef, msg_hidden) -> ReLU -> Linear(msg_hidden, msg_dim) in front of the GRU, whose
     weight_ih is then [3D, msg_dim].  msg_dim must be a multiple of 4 and needs use_memory; msg_hidden > 0 (the reference
     takes (3D+Ef)/2) and is ignored with msg_dim == 0.  Appended (abi 6, additive): a config built from the ten fields above
     with the rest zero is the identity model, bit for bit. */
  int32_t msg_dim;
  int32_t msg_hidden;
} pfo_tgn_config;

/* flat parameter layout (element offsets into the fp32 parameter / gradient buffers) */
typedef struct pfo_tgn_layer_layout {
  int64_t wq, wk, wv, b_in, wo, bo, w1, b1, w2, b2; /* attention_models.{l}: MHA in/out proj + MergeLayer */
} pfo_tgn_layer_layout;
typedef struct pfo_tgn_layout {
  int64_t time_w, time_b;                   /* time_encoder.w.{weight,bias} */
  int64_t gru_w_ih, gru_w_hh, gru_b_ih, gru_b_hh; /* memory_updater.memory_updater.* (-1 without memory) */
  pfo_tgn_layer_layout layer[PFO_MAX_LAYERS];
  int64_t total;
  /* message_function.mlp.{0,2}.{weight,bias}: [msg_hidden, 3D+Ef], [msg_hidden], [msg_dim, msg_hidden], [msg_dim]; -1 without
     the MLP.  The block sits right behind the GRU's and in front of layer[0] (its gradients finish last, with the GRU's:
     pfo_tgn_grad_split), each tensor at an offset that is a multiple of 4 floats. */
  int64_t mlp_w1, mlp_b1, mlp_w2, mlp_b2;
} pfo_tgn_layout;

int pfo_tgn_param_layout(const pfo_tgn_config* cfg, pfo_tgn_layout* out);
/* bytes of scratch pfo_tgn_forward/backward need for (cfg.max_roots, cfg.max_neighbors) */
int64_t pfo_tgn_workspace_bytes(const pfo_tgn_config* cfg);

/* device-resident model state; all caller-owned */
typedef struct pfo_tgn_state {
  const int64_t* indptr; const int32_t* adj_nbr; const int32_t* adj_eidx; const double* adj_ts; /* CSR (K1) */
  const float* node_feat;   /* [n_nodes,D]  tgn.py:35 */
  const float* edge_feat;   /* [E+1,Ef] z-scored, tgn.py:38-41 */
  float* memory;            /* [n_nodes,D]  modules/memory.py:28 */
  float* last_update;       /* [n_nodes]    modules/memory.py:30 */
  float* msg_table;         /* [n_nodes,3D+Ef] last pending raw message per node */
  float* msg_time;          /* [n_nodes] */
  uint8_t* has_msg;         /* [n_nodes] */
  const float* params;      /* flat, pfo_tgn_layout */
  /* Parameter cache (optional, abi 3): a caller-owned device buffer of pfo_tgn_pcache_bytes(cfg) bytes that holds
     everything the step derives from the PARAMETERS alone - the composite weights of every layer (Wqk, cqk, W1ov^T, the
     fc2-folded forms), cos(b) and the fp16 weight images of all contractions incl. the GRU's.  The reference re-reads
     nn.Linear weights per batch and recomputes nothing (tgn.py:219-327); here that work is ~15 small dependent launches,
     so it is done once per parameter VERSION: with pcache_valid == 0 pfo_tgn_forward builds the cache (side stream, as it
     did per step before), with pcache_valid != 0 it launches none of it.  The caller owns the validity: it must pass 0
     after anything wrote `params` (optimizer step, load_state_dict ...) unless pfo_tgn_refresh ran since.  pfo_tgn_backward
     reads the composites from the same buffer: parameters must not change between a forward and its backward.
     The buffer must be ZERO-INITIALISED by the caller when it is allocated (padding rows / columns of the composites are never
     written).  NULL: the composites live in the workspace and are rebuilt by every forward. */
  void* pcache;
  int32_t pcache_valid;
} pfo_tgn_state;

typedef struct pfo_tgn_batch {
  const int32_t* roots;     /* [R] = [src | dst | (p_pos) | neg]   tgn.py:121 / :235 */
  const double* root_ts;    /* [R] timestamps, negatives repeat their interaction's time (tgn.py:123-124,238-239) */
  int32_t R, K;
  int32_t uniform;          /* 0 most-recent, 1 injected draws, 2 Philox */
  const int64_t* const* draws; /* HOST array of n_layers device pointers (level L..1), mode 1 only */
  uint64_t seed, offset;
  float dropout_p;          /* attention-weight dropout, 0 in eval / parity mode (temporal_attention.py:28-32) */
  int32_t training;         /* keep what backward needs */
  const int32_t* extra_nodes; /* [n_extra] nodes whose lazily-updated memory is needed although they are not
                                 embedded here: data-parallel ranks pass the GLOBAL batch's positives so that
                                 pfo_tgn_update_state can persist all of them; may be NULL */
  int32_t n_extra;
  const uint64_t* offset_dev; /* optional device word ADDED to `offset` by every kernel that draws random numbers (dropout
                                 masks, Philox neighbour draws).  A step captured into a HIP graph keeps its kernel
                                 arguments: the per-step stream position then lives here and is advanced on the device */
  int32_t deterministic;    /* != 0: pfo_tgn_backward is bitwise reproducible run to run.  The two order-dependent sums of the
                                 default path - float atomics into the level-0 gradient rows, fp64 atomics into the time-encoder
                                 partial bins - become order-free: the rows are added as 2^-40 fixed-point int64 (integer addition
                                 is associative), the partials go to one slab row per workgroup and are folded in row order.
                                 Costs ~4 % of a C2 step (8-byte atomics); every other sum of the step is ordered already */
  int32_t prepared;         /* != 0: pfo_tgn_prepare already ran for this batch on this workspace (and the caller's stream is
                                 ordered behind it): pfo_tgn_forward skips the frontier sampling, the compaction and the row pack */
  /* optional: the interactions whose state update (pfo_tgn_update_state's arguments: the GLOBAL batch's src / dst / time /
     edge index, upd_B of them) pfo_tgn_forward performs ITSELF - on its side stream, behind the lazy GRU, beside layer 1,
     joined by the event the call's layer 2 waits for anyway: two small launches leave the critical path.  Taken with
     use_memory and n_layers >= 2; otherwise (upd_src NULL, one layer, no memory) the caller calls pfo_tgn_update_state. */
  const int32_t* upd_src; const int32_t* upd_dst; const double* upd_ts; const int32_t* upd_eidx; int32_t upd_B;
  /* Optional INJECTED dropout decisions (parity tests against masks captured from the reference, like `draws` for the uniform
     sampler): dropout_keep[L - l] for layer l (same order as `draws`: the roots' level first) is a device array u8 [n_l, K],
     bit h of entry (n, j) = the attention weight of key slot j / head h of instance n is KEPT; null = the step's own Philox
     draws.  Only read when dropout_p > 0 and training != 0. */
  const uint8_t* const* dropout_keep;
  /* Optional hipEvent_t pfo_tgn_backward records on the caller's stream right behind layer 1's d ctx' contraction, i.e. when
     the layer-1 attention backward - the longest kernel of the step, ~1/3 of it - is about to start.  A caller that prepares
     the NEXT batch (pfo_tgn_prepare on another stream: sampling, compaction, row pack - small latency-bound launches) makes
     that stream wait for this event, so the preparation runs beside the one phase of the step that hides it. */
  void* mid_event;
  int32_t defer_join;       /* pfo_tgn_backward: != 0 leaves the END of the backward on the library's first side stream: the
                               caller's stream is NOT made to wait for the side streams' last launches (the chain back to the
                               layer-1 projection weights, the time-encoder fold: ~40 us after the caller's stream has run dry at
                               C2); instead that side stream waits for the caller's stream, so "everything of this backward" is
                               complete THERE.  The caller must then take the optimizer step with pfo_tgn_adam_side (same side
                               stream) or call pfo_tgn_join before it touches gradients or parameters on its own stream.  The
                               next pfo_tgn_forward joins by itself - behind its neighbour sampling, which reads neither. */
  int32_t seg_in_forward;   /* training calls whose state update runs inside the forward (upd_* given): != 0 lets the forward also
                               queue - on its side stream, beside layer 1 - what the backward's layer-1 kernels need from it and
                               that depends on the sampled levels alone (the instance groups per touched row, the cleared
                               level-0 gradient table); the backward (same batch struct) then forks nothing at its start and
                               waits for nothing in front of its attention kernel */
  int32_t mid_event_late;   /* != 0: record it BEHIND the layer-1 attention backward instead - the preparation then runs beside the
                               backward's serial tail (per-row sums, the touched-table contractions, the GRU's weight gradients:
                               small launches that leave most of the chip idle) */
} pfo_tgn_batch;

/* The part of pfo_tgn_forward that depends on neither parameters nor gradients - frontier sampling (utils.py:163-219 per level,
 * embedding_module.py:125), compaction of the touched nodes, the packed copies of their memory / message rows (tgn.py:251) - on
 * ANY stream.  A training loop issues it for batch n+1 on a second stream as soon as batch n's forward (whose state update
 * writes the tables the pack reads) is queued, into a second workspace: it then runs beside batch n's backward, and batch
 * n+1's forward (batch.prepared = 1, its stream made to wait for this one) starts at the GRU.  The reference does the same
 * work on the host between batches (main.py:190-207 + the neighbour finder inside the model call). */
int pfo_tgn_prepare(const pfo_tgn_config* cfg, const pfo_tgn_state* st, const pfo_tgn_batch* batch, void* workspace,
                    void* stream);

/* Lazy memory update for touched nodes (tgn.py:251, memory_updater.py:35-53) + L-layer temporal graph
 * attention (embedding_module.py:76-175, temporal_attention.py:34-90).  emb_out f32[R,D]. */
int pfo_tgn_forward(const pfo_tgn_config* cfg, const pfo_tgn_state* st, const pfo_tgn_batch* batch,
                    void* workspace, float* emb_out, void* stream);
/* Gradients of everything pfo_tgn_forward (training=1) computed, given d_emb f32[R,D]; ACCUMULATES into grad (flat). */
int pfo_tgn_backward(const pfo_tgn_config* cfg, const pfo_tgn_state* st, const pfo_tgn_batch* batch,
                     void* workspace, const float* d_emb, float* grad, void* stream);
/* The same with two options for the training loop:
 *   zero_grad_first  != 0: `grad` is cleared by this call (on its side stream, off the critical path) before anything is added -
 *                          replaces the caller's memset of the 6 MB flat buffer (optimizer.zero_grad(), main.py:386)
 *   top_ready_event  (hipEvent_t as void*, may be NULL): recorded, on an internal stream, at the point where every gradient of
 *                          the TOP layer's parameter block - elements [pfo_tgn_grad_split(cfg), layout.total) of `grad` - is
 *                          final, ~half a step before the call's last kernel: a data-parallel caller makes its communication
 *                          stream wait for it and all-reduces that block beside the rest of the backward.  Only
 *                          with n_layers >= 2 (pfo_tgn_grad_split returns layout.total otherwise and the event is not recorded).
 *   mean_src / mean_n / mean_out (may be NULL / 0 / NULL): out[0] = mean(mean_src[0 .. mean_n)) is taken on this call's side
 *                          stream, beside the backward, and is complete when the call's work is (pfo_bpr_loss_parts leaves the
 *                          loss's final reduction to it: the loss VALUE is not an input of the backward) */
int pfo_tgn_backward_ev(const pfo_tgn_config* cfg, const pfo_tgn_state* st, const pfo_tgn_batch* batch,
                        void* workspace, const float* d_emb, float* grad, int32_t zero_grad_first, void* top_ready_event,
                        const float* mean_src, int64_t mean_n, float* mean_out, void* stream);
int pfo_tgn_grad_split(const pfo_tgn_config* cfg, int64_t* split);
/* Persist memory for the positives, clear their pending messages, build and store the new raw messages with
 * last-wins semantics (tgn.py:290-317, memory_updater.py:18-33, memory.py:35-37,73-75, tgn.py:357-378).
 * src/dst i32[B], ts f64[B], eidx i32[B]; needs the workspace of the forward call that preceded it. */
int pfo_tgn_update_state(const pfo_tgn_config* cfg, const pfo_tgn_state* st, const int32_t* src, const int32_t* dst,
                         const double* ts, const int32_t* eidx, int32_t B, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * Serving write path: advance memory, last_update and the pending-message tables over a chronological log WITHOUT
 * embedding anything - the write-only counterpart of pfo_recommend_topk.  The log src/dst i32[N], ts f64[N], eidx i32[N]
 * (device pointers; node ids in [0, n_nodes), eidx rows of edge_feat) is walked in ceil(N / B) batches of B interactions,
 * the last one shorter, queued back to back from the host side of this call.  Per batch (positives P = src u dst):
 *   1. every X in P with has_msg[X]:  memory[X] = GRUCell(msg_table[X], memory[X]),  last_update[X] = msg_time[X]
 *      (tgn.py:295, memory_updater.py:18-33); other positives keep both bit for bit; a node named twice is updated once
 *   2. pfo_tgn_update_state's message store: event e = side * B + i ascending, the last event per node wins; both memory
 *      reads see the state after step 1 for the whole batch (tgn.py:302-317, 357-378)
 * Batch k+1 sees the state batch k left: batch boundaries are part of the semantics, B is not a tuning knob.
 * Nothing else is written (parameters, gradients, optimizer state).  Launches per batch: 4 - row selection (the distinct
 * positives that hold a message, compacted), the step's fused GRU launch in its gather form over exactly those rows, persist,
 * message store - and 5 when 2 B > 16384 (the store's winner pass).  Per call in front of them: one clear of the row
 * selection's stamp table and, when st->pcache_valid is not set, ONE launch that builds the GRU's two weight images into the
 * workspace (with a valid parameter cache they are taken from st->pcache).
 * Everything runs on `stream` (the call first joins work pfo_tgn_adam_side left on the library's side stream): capturable.
 * The CSR pointers of `st` are not read and may be NULL.  N == 0 queues nothing.  PFO_ERR_INVALID: cfg->use_memory == 0,
 * B < 1 (or >= 2^30), N < 0, workspace_bytes < pfo_tgn_observe_workspace_bytes(cfg, B) (which returns -1 for a bad cfg / B).
 */
int64_t pfo_tgn_observe_workspace_bytes(const pfo_tgn_config* cfg, int32_t B);
int pfo_tgn_observe(const pfo_tgn_config* cfg, const pfo_tgn_state* st, const int32_t* src, const int32_t* dst,
                    const double* ts, const int32_t* eidx, int64_t N, int32_t B, void* workspace, int64_t workspace_bytes,
                    void* stream);

/* ------------------------------------------------------------------------------------------
 * Serving ingest: rows of RAW edge features, z-scored with the model's FROZEN column statistics, appended to the edge-feature
 * table (abi 6, additive).  table[row0 + i][j] = (raw[i][j] - mean[j]) / stdv[j] for i < m, j < Ef - numpy's fp32
 * `ef -= mean; ef /= std`: one correctly rounded subtraction, then one correctly rounded division (no FMA, no reciprocal), so a
 * zero-variance column yields inf / NaN exactly where numpy does.  raw f32[m, Ef], mean / stdv f32[Ef], table f32[cap, Ef]: device
 * pointers, rows contiguous; Ef is arbitrary (no alignment is assumed).  One launch on `stream`; rows outside [row0, row0 + m)
 * are not touched.  m == 0 queues nothing.  PFO_ERR_INVALID - nothing is written: m < 0, Ef < 1, row0 outside [0, cap],
 * row0 + m > cap, a null pointer with m > 0.
 */
int pfo_edge_rows_append(const float* raw, const float* mean, const float* stdv, int64_t m, int32_t Ef, float* table,
                         int64_t row0, int64_t cap, void* stream);
/* Retention of the edge-feature table (abi 6, additive).  The table is shared between finders, so the decision is taken over
 * all of them: row r >= 1 is RELEASED iff some expired adjacency entry (ts < cutoff) names r and no surviving one does; rows
 * nobody names stay, row 0 always stays.  Surviving rows keep their order and are renumbered densely.
 *   pfo_edge_rows_mark    : one call per finder over its adjacency as it was BEFORE the expiry (eidx i32[n], ts f64[n]):
 *                           flags[eidx[i]] |= (ts[i] < cutoff ? 1 : 2).  flags i32[n_rows], zero before the first call; entries
 *                           outside [0, n_rows) are ignored.
 *   pfo_edge_rows_plan    : remap i32[n_rows] = the exclusive scan of the keep flags, -1 for released rows (remap[0] = 0);
 *                           *n_keep (device) = the new row count.  Two launches; scratch: pfo_edge_rows_plan_scratch_bytes.
 *   pfo_edge_rows_compact : kept rows move down to remap[r] inside the table's own storage THROUGH tmp f32[n_keep, Ef] (gather
 *                           into tmp, stream-ordered copy back: no overlapping in-place copy); rows [n_keep, n_rows) are zeroed.
 *                           n_keep == n_rows queues nothing.
 *   pfo_eidx_remap        : eidx[i] = remap[eidx[i]] in place, for every finder that took part.
 * PFO_ERR_INVALID - nothing is queued: bad sizes, a non-finite cutoff, a null pointer, a short scratch.
 */
int pfo_edge_rows_mark(const int32_t* eidx, const double* ts, int64_t n, double cutoff, int64_t n_rows, int32_t* flags,
                       void* stream);
int64_t pfo_edge_rows_plan_scratch_bytes(int64_t n_rows);
int pfo_edge_rows_plan(const int32_t* flags, int64_t n_rows, int32_t* remap, int32_t* n_keep, void* scratch,
                       int64_t scratch_bytes, void* stream);
int pfo_edge_rows_compact(float* table, int64_t n_rows, int64_t n_keep, int32_t Ef, const int32_t* remap, float* tmp,
                          void* stream);
int pfo_eidx_remap(int32_t* eidx, int64_t n, const int32_t* remap, int64_t n_rows, void* stream);

/* ------------------------------------------------------------------------------------------
 * Erasure by node (abi 6, additive): the sibling of the retention calls, by node instead of by time.  gone u8[n_nodes] on the
 * device, 1 = forgotten.  Entry i of row v is DROPPED iff gone[v] or gone[adj_nbr[i]]; a neighbour id outside [0, n_nodes)
 * counts as not gone.  The survivors of a row are no suffix and rows are skewed, so every pass runs one lane per ENTRY.
 *   pfo_nodes_flag           : gone = 0, then gone[ids[j]] = 1 for ids i32[m]; ids outside [1, n_nodes) are skipped (node 0 is
 *                              the padding node), duplicates are fine.  A memset and one launch (m == 0: the memset alone).
 *   pfo_csr_forget_plan      : keep u8[total] = 1 for an entry that stays; new_pos i64[total + 1] = the exclusive scan of keep
 *                              over the flat entries (new_pos[total] = the surviving total); new_indptr i64[n_nodes + 1] =
 *                              new_pos at the row starts - the exclusive scan of the kept count per row - so
 *                              new_indptr[n_nodes] is the surviving total, which the caller reads back to size the output.
 *                              Three launches; scratch holds pfo_csr_forget_scratch_bytes(n_nodes, total) bytes.  total == 0:
 *                              new_indptr and new_pos[0] are zeroed, adj_nbr and keep may be NULL.
 *   pfo_csr_forget_copy      : entry i with keep[i] goes to position new_pos[i] of new arrays of `total` entries: the old order
 *                              inside every row, equal to boolean-masking the flat arrays with keep, bit for bit (timestamps
 *                              keep their bits).  One launch; total == 0 queues nothing.
 *   pfo_edge_rows_mark_nodes : the by-node form of pfo_edge_rows_mark, one call per finder over its adjacency as it was BEFORE
 *                              the removal: flags[eidx[i]] |= (dropped ? 1 : 2); entries outside [0, n_rows) are ignored.
 *                              pfo_edge_rows_plan / _compact and pfo_eidx_remap then run as they stand.  n == 0 queues nothing.
 *   pfo_node_rows_reset      : ONE launch; every row v with gone[v] returns to what a new node holds - memory f32[., D],
 *                              last_update f32, msg_table f32[., M], msg_time f32, has_msg u8 and the node-feature row
 *                              f32[., Dn] to 0, the holdings ledger's hold_idx i32[., W] to -1, hold_len i32 to 0 and
 *                              hold_time f64 to -inf.  Every table is optional (NULL: skipped); no row width needs a multiple
 *                              of 4; rows that are not flagged keep every bit.
 * PFO_ERR_INVALID - all checks are made on the host and nothing is queued: bad sizes (n_nodes < 1, a negative count, counts of
 * 2^31 and above, total > old_total, a table given with a width < 1), a null pointer where one is needed, a short scratch.
 */
int pfo_nodes_flag(const int32_t* ids, int64_t m, int64_t n_nodes, uint8_t* gone, void* stream);
int64_t pfo_csr_forget_scratch_bytes(int64_t n_nodes, int64_t total);
int pfo_csr_forget_plan(const int64_t* indptr, const int32_t* adj_nbr, int64_t n_nodes, int64_t total, const uint8_t* gone,
                        uint8_t* keep, int64_t* new_pos, int64_t* new_indptr, void* scratch, int64_t scratch_bytes, void* stream);
int pfo_csr_forget_copy(const int32_t* old_nbr, const int32_t* old_eidx, const double* old_ts, int64_t old_total,
                        const uint8_t* keep, const int64_t* new_pos, int64_t total, int32_t* new_nbr, int32_t* new_eidx,
                        double* new_ts, void* stream);
int pfo_edge_rows_mark_nodes(const int64_t* indptr, const int32_t* adj_nbr, const int32_t* adj_eidx, int64_t n, int64_t n_nodes,
                             const uint8_t* gone, int64_t n_rows, int32_t* flags, void* stream);
int pfo_node_rows_reset(const uint8_t* gone, int64_t n_nodes, float* memory, int32_t D, float* last_update, float* msg_table,
                        int32_t M, float* msg_time, uint8_t* has_msg, float* node_feat, int32_t Dn, int32_t* hold_idx, int32_t W,
                        int32_t* hold_len, double* hold_time, void* stream);

/* ------------------------------------------------------------------------------------------
 * Holdings ledger (abi 6, additive): per node row the portfolio its newest interaction record carried.  hold_idx i32[n_nodes, W]
 * STOCK indices padded with -1 (the packed form of port_idx everywhere else; the item node of stock s is s + upper_u + 1),
 * hold_len i32[n_nodes] valid leading entries, hold_time f64[n_nodes] the record's time.  All pointers are device pointers.
 *
 * pfo_holdings_store: for e = 0..N-1 in input order, u = src[e]: skipped unless 1 <= u < n_nodes; L = clamp(port_len[e], 0,
 *   min(W, port_stride)); hold_idx[u, :L] = port_idx[e, :L] (row stride port_stride, entries verbatim), hold_idx[u, L:] = -1,
 *   hold_len[u] = L, hold_time[u] = ts[e].  Per user the LAST event of the call wins, on every run and for every launch
 *   geometry: a cleared stamp table, atomicMax(stamp[u], e + 1), and the event that finds its own stamp copies the row with one
 *   lane per element - three stream-ordered nodes (memset, two kernels), no workgroup waits for another.  Rows of nodes the
 *   call does not name keep every bit.  scratch: pfo_holdings_store_scratch_bytes(n_nodes, N) bytes (-1 for bad sizes), its
 *   content on entry is irrelevant.  port_idx may be NULL when port_stride == 0.
 * pfo_holdings_gather: for q < U, u = users[q], ok = 0 <= u < n_nodes: port_idx_out[q, :] = ok ? hold_idx[u, :] : -1,
 *   port_len_out[q] = ok ? hold_len[u] : 0, and - unless excl_pos_out is NULL - excl_pos_out[q, j] = the position in items
 *   i32[I] (distinct node ids) of node hold_idx[u, j] + upper_u + 1 if ok, j < hold_len[u] and that node is a candidate, else
 *   -1 (the stock index is range-checked before the addition).  pos_scratch i32[n_nodes] needs no initialisation and may be
 *   kept between queries: pos_scratch[items[i]] = i is scattered, and an entry p is trusted only if 0 <= p < I and
 *   items[p] names the node - another list's positions are never seen.  Two launches (one when excl_pos_out is NULL: items
 *   and pos_scratch are then not read and may be NULL).  Outputs: i32[U, W], i32[U], i32[U, W].
 * PFO_ERR_INVALID - checked before anything is read, nothing is written: W outside [1, 256], N outside [0, 2^31), I outside
 * [1, PFO_RECOMMEND_MAX_ITEMS], n_nodes < 1 (or >= 2^31), port_stride < 0, U < 0; then a null pointer, a short scratch.
 * N == 0 / U == 0 queue nothing and return PFO_OK.
 */
int64_t pfo_holdings_store_scratch_bytes(int64_t n_nodes, int64_t N);
int pfo_holdings_store(const int32_t* src, const int32_t* port_idx, const int32_t* port_len, int32_t port_stride, const double* ts,
                       int64_t N, int32_t* hold_idx, int32_t* hold_len, double* hold_time, int64_t n_nodes, int32_t W, void* scratch,
                       int64_t scratch_bytes, void* stream);
int pfo_holdings_gather(const int32_t* users, int64_t U, const int32_t* hold_idx, const int32_t* hold_len, int64_t n_nodes, int32_t W,
                        const int32_t* items, int32_t I, int32_t upper_u, int32_t* pos_scratch, int32_t* port_idx_out,
                        int32_t* port_len_out, int32_t* excl_pos_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Holdings from trades (abi 6, additive): the ledger's second writer - buys and sells applied to the rows in event order.
 * Tables as above, and optionally hold_qty f64[n_nodes, W]: the share count of every slot, 0.0 at and behind hold_len.
 *
 * pfo_holdings_apply: for e = 0..N-1 in input order, u = src[e] i32, s = stock[e] i32, side[e] i32, t = ts[e] f64:
 *   - valid iff 1 <= u < n_nodes, s >= 0, side is +1 (buy) or -1 (sell) and - when hold_qty AND qty are given - q = qty[e] is
 *     finite and > 0.  An invalid event is skipped whole.  With hold_qty and qty NULL every q is 1.0; without hold_qty, qty is
 *     not read.
 *   - L = clamp(hold_len[u], 0, W); j = the FIRST position of hold_idx[u, :L] that holds s (rows the snapshot writer seeded
 *     may hold duplicates and negative entries).
 *   - buy, present: hold_qty[u, j] += q (one fp64 add), nothing without quantities.  Buy, absent, L < W: hold_idx[u, L] = s,
 *     hold_qty[u, L] = q, hold_len[u] = L + 1.  Buy, absent, row full: the row is unchanged, counters[0] (overflow) += 1.
 *   - sell, absent: unchanged, counters[1] (unmatched) += 1.  Sell, present: with quantities rem = hold_qty[u, j] - q; rem > 0:
 *     hold_qty[u, j] = rem.  Otherwise (always without quantities) the position is closed: entries j+1 .. L-1 of hold_idx and
 *     hold_qty move one slot to the front, slot L-1 becomes (-1, 0.0), hold_len[u] = L - 1 - a row lists positions oldest first.
 *   - every valid event: hold_time[u] = t (nothing is compared with the stored time).
 *   Rows of users no valid event names keep every bit; the inputs are never written; counters i64[2] (nullable) are ADDED to.
 *   The result is that loop's on every run and for every launch geometry: the event indices are grouped by user with a stable
 *   radix (8 bits a pass, ceil(log256(n_nodes)) passes; N <= 1024 in one launch), then one wavefront walks a user's chain over
 *   the row held in registers and writes it once; only the two integer counters meet in atomics.  A user with many events
 *   in one call is walked serially.  scratch: pfo_holdings_apply_scratch_bytes(n_nodes, N) bytes (-1 for bad sizes), content
 *   on entry irrelevant.
 * PFO_ERR_INVALID - checked before anything is read, nothing is written: W outside [1, 256], N outside [0, 2^31), n_nodes
 * outside [1, 2^31); then a null pointer (qty, hold_qty and counters may be NULL), a short scratch.  N == 0 queues nothing.
 */
int64_t pfo_holdings_apply_scratch_bytes(int64_t n_nodes, int64_t N);
int pfo_holdings_apply(const int32_t* src, const int32_t* stock, const int32_t* side, const double* qty, const double* ts, int64_t N,
                       int32_t* hold_idx, int32_t* hold_len, double* hold_time, double* hold_qty, int64_t n_nodes, int32_t W,
                       int64_t* counters, void* scratch, int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Position weights from the ledger (abi 6, additive): the rows port_w of the weighted recommend entries, aligned with
 * pfo_holdings_gather's port_idx_out.  For q < U, u = users[q], L = clamp(hold_len[u], 0, W) when 0 <= u < n_nodes, else 0:
 *   w_out[q, j] = 0.0                                         for j >= L;
 *   mode 0 (shares): hold_qty[u, j]                           for j < L;
 *   mode 1 (value):  hold_qty[u, j] * last_close[hold_idx[u, j]] (one rounded product) for j < L and the stock in [0, n_stocks),
 *                    0.0 for a stock outside it.  A stock never quoted has last_close NaN: its weight is NaN, and the ranking
 *                    kernel leaves it out.
 * Every slot of w_out f64[U, W] is written; one launch, one lane per slot; every index read from device memory is range-checked
 * before use.  last_close f64[>= n_stocks].  PFO_ERR_INVALID before any pointer is looked at: W outside [1, 256], U < 0,
 * n_nodes < 1 (or >= 2^31), n_stocks < 0, mode outside {0, 1}; then (U > 0) a null pointer - hold_qty always, last_close with
 * mode 1.  U == 0 queues nothing.
 */
int pfo_holdings_gather_weights(const int32_t* users, int64_t U, const int32_t* hold_idx, const int32_t* hold_len, const double* hold_qty,
                                int64_t n_nodes, int32_t W, const double* last_close, int64_t n_stocks, int32_t mode, double* w_out,
                                void* stream);

/* ------------------------------------------------------------------------------------------
 * History gather (abi 6, additive): what a user has interacted with, read from the temporal adjacency the finder keeps on the
 * device - the time-sorted CSR indptr i64[n_nodes + 1], adj_nbr i32, adj_ts f64.  All pointers are device pointers.
 *
 * pfo_history_gather: for q < U, u = users[q] i32, t = ts[q] f64:
 *   - u outside [0, n_nodes) or t not finite: the answer is empty.
 *   - hi = the number of entries of row u with adj_ts < t: strict, compared in fp64 on the stored fp64 timestamps (the rule of
 *     pfo_csr_expire_plan; none of the sampler's fp32 casts apply).
 *   - lo = the number of entries with adj_ts < since[q] (an entry AT since[q] is inside); 0 when since is NULL or since[q] is
 *     NaN.  With max_scan > 0: lo = max(lo, hi - max_scan) - at most the max_scan newest entries are looked at.  hi <= lo: empty.
 *   - the window is walked NEWEST FIRST, e = hi - 1, hi - 2, .., lo (among equal timestamps the later row entry first): a
 *     neighbour met for the first time takes the next free slot while fewer than W are kept; a neighbour met again adds one to
 *     its slot's count; a first meeting when W slots are taken is dropped, and so are its repeats.
 *   node_out  i32[U, W]: the distinct neighbour node ids, newest first, padded with -1;  len_out i32[U]: the slots used;
 *   time_out  f64[U, W] or NULL: the newest timestamp of each kept neighbour, copied bit for bit, padding NaN;
 *   count_out i32[U, W] or NULL: the entries of the window that name it, padding 0;
 *   pos_out   i32[U, W] or NULL: the position of the node in items i32[I] (distinct node ids), else -1 - through pos_scratch
 *             i32[n_nodes] exactly as in pfo_holdings_gather: pos_scratch[items[i]] = i is scattered (ids outside [0, n_nodes)
 *             skipped), an entry p is trusted only if 0 <= p < I and items[p] names the node; no initialisation needed;
 *   stock_out i32[U, W] or NULL: node - upper_u - 1 when that lies in [0, 2^31), else -1 (checked in 64 bits: nothing wraps).
 *   Every slot of every requested output row is written, padding included; nothing else is written.  One user per 64-thread
 *   workgroup, bounds by a wave-wide 64-ary search, the walk in chunks of 64 entries; once W are kept the walk goes on only
 *   for count_out.  Integer arithmetic only: the same answer on every run.  One launch, two with pos_out (the scatter).
 * PFO_ERR_INVALID - checked before any pointer is looked at, nothing is queued: W outside [1, PFO_HISTORY_MAX_WIDTH], U outside
 * [0, INT64_MAX / PFO_HISTORY_MAX_WIDTH] (the output rows are indexed in 64 bits),
 * n_nodes < 1 (or >= 2^31), max_scan < 0, pos_out given and I outside [1, PFO_RECOMMEND_MAX_ITEMS]; then a null pointer that is
 * needed (items and pos_scratch only with pos_out; since, time_out, count_out, pos_out, stock_out may be NULL).  U == 0 queues
 * nothing and returns PFO_OK.
 */
#define PFO_HISTORY_MAX_WIDTH 256
int pfo_history_gather(const int64_t* indptr, const int32_t* adj_nbr, const double* adj_ts, int64_t n_nodes, const int32_t* users,
                       const double* ts, const double* since, int64_t U, int32_t W, int64_t max_scan, const int32_t* items,
                       int32_t I, int32_t* pos_scratch, int32_t upper_u, int32_t* node_out, int32_t* len_out, double* time_out,
                       int32_t* count_out, int32_t* pos_out, int32_t* stock_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Price ledger (abi 6, additive): the log-return table of the mean-variance rank kept on the device and grown by the day.
 * returns f64[day_cap, stock_cap, n_ret]: the day axis is a ring of slots, a slot holds stock_cap rows of n_ret doubles, row s
 * of a day is the window of stock s's n_ret newest log-returns as of that day, oldest first.  pfo_mv_select,
 * pfo_recommend_mv_topk and pfo_recommend_basket_topk read the table unchanged with n_days = day_cap, n_stocks = stock_cap and
 * day_idx = the SLOT.  A row never quoted, and every row at or behind n_stocks, is all zeros: a constant series has y = 0/0, so
 * by the NaN rule of those kernels such a stock is not admissible until its window holds two different closes.  day_keys
 * i64[day_cap]: the key of each slot, strictly increasing over the live slots in ring order; last_close f64[stock_cap]: NaN
 * until a stock is first quoted.  All pointers are device pointers.
 *
 * pfo_returns_append_day: writes rows [0, n_stocks) of slot new_slot and day_keys[new_slot] = day_key, one launch, one lane per
 *   element, nothing else is written (rows [n_stocks, stock_cap) of the slot keep their bits).  For s < n_stocks:
 *     R[new, s, j] = R[prev, s, j + 1] for j < n_ret - 1, copied bitwise (+0 when prev_slot == -1: the first day);
 *     c = the close of s: dense (stamp NULL) closes[s] for s < n_closes; sparse closes[stamp[s] - 1] when 1 <= stamp[s] <=
 *       n_closes (the table pfo_returns_scatter_closes left); otherwise not quoted.  A close that is not positive and finite
 *       (NaN included) is "not quoted";
 *     quoted and last_close[s] not NaN: R[new, s, n_ret - 1] = log(c / last_close[s]) - the IEEE fp64 quotient, then log;
 *       otherwise +0.  Quoted: last_close[s] = c; not quoted: last_close[s] is carried forward.
 *     quot_out f64[n_stocks] (may be NULL, for tests): the quotient the logarithm was taken of, NaN where none was.
 *   prev_slot must differ from new_slot (the copy is not in place), so day_cap >= 2.
 * pfo_returns_scatter_closes: the sparse form (stocks i32[m], closes f64[m]) -> stamp i32[n_stocks]: cleared, then
 *   atomicMax(stamp[s], p + 1) over the positions p whose index lies in [0, n_stocks) and whose close is positive and finite;
 *   the others are skipped.  Among repeated indices the LAST valid position wins on every run and for every launch geometry
 *   (the scheme of pfo_holdings_store).  A memset and one launch; stamp's content on entry is irrelevant, its size is
 *   pfo_returns_scatter_scratch_bytes(n_stocks) (-1 for bad sizes).
 * pfo_day_lookup: slot_out[u] = the slot of the live day whose key is (int64) floor(ts[u] / key_divisor), -1 when the ledger
 *   holds no such day (or ts[u] is not finite): a binary search over the n_days live slots head, head + 1, .. (mod day_cap).
 *   The query kernels give a user whose day is -1 an empty answer and read nothing for it.  One launch.
 * PFO_ERR_INVALID - checked before anything is read, nothing is written: day_cap < 2 (lookup: < 1), n_ret outside [2, 128],
 * stock_cap outside [1, 2^31), n_stocks outside [0, stock_cap], a slot outside the ring, prev_slot == new_slot, m / n_closes
 * outside [0, 2^31), head / n_days outside the ring, a key_divisor that is not positive and finite; then a null pointer, a
 * short scratch.  U == 0 queues nothing.
 */
int64_t pfo_returns_scatter_scratch_bytes(int64_t n_stocks);
int pfo_returns_scatter_closes(const int32_t* stocks, const double* closes, int64_t m, int64_t n_stocks, int32_t* stamp,
                               int64_t stamp_bytes, void* stream);
int pfo_returns_append_day(double* returns, int32_t day_cap, int64_t stock_cap, int32_t n_ret, int32_t prev_slot, int32_t new_slot,
                           int64_t n_stocks, const double* closes, int64_t n_closes, const int32_t* stamp, double* last_close,
                           int64_t* day_keys, int64_t day_key, double* quot_out, void* stream);
int pfo_day_lookup(const double* ts, int64_t U, const int64_t* day_keys, int32_t day_cap, int32_t head, int32_t n_days,
                   double key_divisor, int32_t* slot_out, void* stream);

/* diagnostics for tests: copies of internals of the last forward (device pointers into the workspace) */
typedef struct pfo_tgn_debug {
  const int32_t* n_touched;  /* [1] */
  const int32_t* touched_ids;/* [n_touched] */
  const float* h0_table;     /* [n_touched,D] layer-0 features memory'+node_feat (embedding_module.py:98) */
  const int32_t* slot;       /* [n_nodes] */
  /* operands and results of the two largest weight-gradient contractions of the last backward (valid until the workspace's
     next forward): parity tests re-contract the SAME fp32 operands in fp64 (per-element evidence for the split contraction) */
  const int32_t* n_core;     /* [1] table rows the step's levels reference (the GRU backward's row count) */
  const float* l1_ctx;       /* [n_1, H*Cp]   layer-1 context rows ctx' (a operand of dW1ov)                     */
  const float* l1_dh1;       /* [n_1, D]      d loss / d (layer-1 fc1 pre-activation) (b operand)               */
  const float* l1_dW1ovT;    /* [H*Cp, D]     = ctx'^T dh1                                                      */
  const float* gru_dgi;      /* [n_core, 3D]  d loss / d (GRU input-side pre-activations) (a operand of dW_ih)  */
  const float* gru_msg_rows; /* [n_core, 3D+Ef] packed message rows (b operand); dW_ih lands in the gradient buffer */
  int32_t Cp;                /* per-head row stride of ctx' */
  /* the message MLP's activations of the last forward (NULL with msg_dim == 0): rows follow touched_ids */
  const float* mlp_hid;      /* [n_touched, msg_hidden] relu(W1 raw + b1) */
  const float* mlp_out;      /* [n_touched, msg_dim]    W2 hid + b2: the GRU's input rows */
} pfo_tgn_debug;
int pfo_tgn_debug_views(const pfo_tgn_config* cfg, void* workspace, pfo_tgn_debug* out);

/* ------------------------------------------------------------------------------------------
 * Explanation query (abi 6, additive): which past interactions an embedding attends to, read from the workspace of the
 * pfo_tgn_forward call that computed it - before that workspace is used again.  `cfg` is the configuration the workspace was
 * carved with, R and K are that call's (cfg->n_layers = L, cfg->n_heads = H).  Nothing of the workspace is written.
 *
 * What is read (level l holds n_l instances: n_L = R, n_(l-1) = n_l (1 + K); all tables have stride K of the call, not
 * max_neighbors): the neighbour ids of level l's instances (behind that level's own n_l nodes in the list the sampler wrote for
 * level l - 1), its edge ids eidx [n_l, K], its dt f32 [n_l, K] (the instance's time minus the edge's time: the value the time
 * encoder saw; every level's instance time is its root's) and the layer's softmax weights attw f32 [n_l, H, K] (before dropout,
 * 0 on padding, all 0 on an instance without a neighbour).
 *
 *   head mean   p_l[n, k] = (sum over h ascending of (double) attw_l[n, h, k]) / (double) H - what nn.MultiheadAttention
 *               returns beside its output.  A slot COUNTS iff its neighbour id is not 0.
 *   hops == 1   root r: the entries are its counting slots k of level L, entry k names node nbr_L[r, k] with weight p_L[r, k],
 *               age dt_L[r, k] and edge eidx_L[r, k].
 *   hops == 2   (attention rollout) for every counting slot j of root r, row = R + r K + j of level L - 1 is that neighbour's
 *               instance; the entries are the paths q = j K + i whose slot i of that row counts: node nbr_(L-1)[row, i],
 *               weight p_L[r, j] * p_(L-1)[row, i] (ONE rounded fp64 product), age and edge of the path's LAST hop
 *               (dt_(L-1)[row, i], eidx_(L-1)[row, i]).  The root's own level-(L-1) row is not part of the rollout.
 *   merge       entries that name the same node become one: weight = the sum of theirs taken sequentially in ascending k / q
 *               from 0.0, count = how many, age = the smallest of theirs, eidx = that entry's (among equal ages the lowest k / q).
 *   order       weight descending (fp64), then age ascending, then node id ascending.
 * All arithmetic is fp64 without contraction; nothing is added out of order: the same input gives the same bits on every run.
 *
 *   node_out i32[R, m] padded with -1;  weight_out f64[R, m] padded with 0.0;  n_valid_out i32[R] = min(m, distinct nodes);
 *   count_out i32[R, m] padded with 0;  age_out f32[R, m] padded with NaN;  eidx_out i32[R, m] padded with -1.
 *   Every slot of every row is written.  A hops == 1 row sums to 1 up to rounding (0 when empty), a hops == 2 row to at most 1.
 *   raw_nbr i32[R, K], raw_w f32[R, H, K], raw_dt f32[R, K], raw_eidx i32[R, K]: copies of level L's tables - all four or all
 *   NULL.  raw_nbr2 i32[R, K, K], raw_w2 f32[R, K, H, K], raw_dt2 f32[R, K, K], raw_eidx2 i32[R, K, K]: level L - 1's rows
 *   R .. R + R K - all four or all NULL, written with hops == 2 only.
 * One launch (csrc/explain.hip), a workgroup per root.  PFO_ERR_INVALID - checked before any pointer is looked at, nothing is
 * queued: a bad configuration, m outside [1, PFO_EXPLAIN_MAX_WIDTH], hops outside [1, min(2, n_layers)], K outside
 * [1, min(PFO_MAX_NEIGHBORS, max_neighbors)], R outside [0, max_roots]; then a null workspace or output, or a raw group given
 * in part.  R == 0 queues nothing and returns PFO_OK.
 */
#define PFO_EXPLAIN_MAX_WIDTH 256
int pfo_tgn_explain(const pfo_tgn_config* cfg, const void* workspace, int32_t R, int32_t K, int32_t hops, int32_t m,
                    int32_t* node_out, double* weight_out, int32_t* n_valid_out, int32_t* count_out, float* age_out,
                    int32_t* eidx_out, int32_t* raw_nbr, float* raw_w, float* raw_dt, int32_t* raw_eidx, int32_t* raw_nbr2,
                    float* raw_w2, float* raw_dt2, int32_t* raw_eidx2, void* stream);

/* debug / test probes of the internal contraction interface (csrc/gemm.hpp).  Every struct mirrors the internal one field
 * for field and every call forwards to the internal launcher unchanged; the comments of gemm.hpp are the contract.  Not part
 * of the drop-in surface: the package's own Python never calls them, the kernel tests do. */
typedef struct pfo_gemm_desc {     /* PfoGemm */
  const float* A[2]; int64_t lda[2]; const int32_t* a_idx[2];
  const float* B[2]; int64_t ldb[2]; const int32_t* b_idx;
  int32_t K[2];
  float* C; int64_t ldc;
  const float* bias;
  const float* row_scale; int64_t rs_ld;
  const uint8_t* row_zero;
  const float* relu_src; int64_t relu_ld;
  const float* add_src; int64_t add_ld; const int32_t* add_idx;
  int32_t M, N;
  const int32_t* m_dev;
  int32_t relu, accumulate, a_kmajor, b_kmajor;
  int32_t batch;
  int64_t a_bs[2], b_bs[2], c_bs, bias_bs, rs_bs;
  float* slabs; int64_t slab_floats;
  const void* b_img; const void* b_img2;
  int32_t bx_force;
} pfo_gemm_desc;
typedef struct pfo_tn_desc {       /* PfoTnProblem */
  const float* A; int64_t lda;
  const float* B; int64_t ldb; const int32_t* b_idx;
  int32_t M, N;
  float* C; int64_t ldc; int32_t c_accumulate;
  float* bias_out; int32_t bias_accumulate;
} pfo_tn_desc;
typedef struct pfo_bimg_desc {     /* PfoBimg */
  const float* src; int64_t ld; int32_t N, K, trans; void* dst;
  int32_t row0, rows_total, last;
  int32_t gate, gate_D;
} pfo_bimg_desc;
typedef struct pfo_gru_desc {      /* PfoGruFused */
  const float* msg_rows; int32_t K_msg;
  const float* h_rows;
  const void* img_ih; const void* img_hh;
  const float* b_ih; const float* b_hh;
  const uint8_t* hm; const int32_t* touched; const float* node_feat;
  float* upd_mem; float* h0_tab; float* gates;
  int32_t D, cap_rows; const int32_t* n_rows;
  int32_t gather;
} pfo_gru_desc;
typedef struct pfo_rank1_desc {    /* PfoRank1 */
  const float* u; int64_t ldu; const float* v; int64_t ldv; int32_t M, N; float* out; int64_t ldo;
  int32_t reps; int64_t u_rs, v_rs;
} pfo_rank1_desc;
typedef struct pfo_sum_slabs_desc { /* PfoSumSlabs */
  float* dst; const float* src; int64_t stride, count; int32_t n_slabs, accumulate;
} pfo_sum_slabs_desc;
int pfo_debug_gemm(const pfo_gemm_desc* g, void* stream);
int pfo_debug_gemm_multi(const pfo_gemm_desc* list, int32_t n, void* stream);
int pfo_debug_gemm_tn_group(const pfo_tn_desc* probs, int32_t n, int32_t K, const int32_t* k_dev, float* slabs, int64_t slab_floats,
                            void* stream);
int64_t pfo_debug_bimg_bytes(int32_t N, int32_t K);
int64_t pfo_debug_gru_img_bytes(int32_t D, int32_t K);
int pfo_debug_bimg(const pfo_bimg_desc* list, int32_t n, void* stream);
int pfo_debug_gru_fused(const pfo_gru_desc* f, void* stream);
/* The MLP message function's forward in one launch (csrc/gemm.hpp PfoMsgMlp / pfo_msg_mlp_fwd_launch): hid = relu(raw W1^T + b1),
 * msg_out = hid W2^T + b2 over cap_rows rows (device count n_rows), W1 [Hm, Mr] and W2 [Md, Hm] as plain pfo_debug_bimg images
 * (N = Hm, K = Mr and N = Md, K = Hm; pfo_debug_bimg_bytes each).  touched != NULL: raw / hm are per-node tables and row m is
 * node touched[m]; NULL: packed rows.  Rows with hm == 0 are not read and give zeros; hid (may be NULL) and msg_out are written
 * for rows < min(cap_rows, *n_rows) only.  Mr % 4 == 0, Md % 4 == 0, 16-byte aligned raw / msg_out / images. */
typedef struct pfo_msg_mlp_desc {  /* PfoMsgMlp */
  const float* raw; int64_t ld_raw;
  const int32_t* touched; const uint8_t* hm;
  const void* img_w1; const void* img_w2;
  const float* b1; const float* b2;
  float* hid; float* msg_out;
  int32_t Mr, Hm, Md, cap_rows; const int32_t* n_rows;
} pfo_msg_mlp_desc;
int pfo_debug_msg_mlp_fwd(const pfo_msg_mlp_desc* f, void* stream);
/* ... and the data path of its backward (PfoMsgMlpBwd / pfo_msg_mlp_bwd_launch): d_m = dgi W_ih (written when not NULL),
 * d_hid = (d_m W2) where hid > 0, exactly 0 elsewhere; dgi [rows, D3], hid [rows, Hm] packed; the images are those of W_ih^T
 * (pfo_debug_bimg with trans = 1, N = Md, K = D3, src = W_ih [D3, Md]) and of W2^T (trans = 1, N = Hm, K = Md, src = W2 [Md, Hm]).
 * Md <= 128 and a multiple of 4, D3 a multiple of 4. */
typedef struct pfo_msg_mlp_bwd_desc {  /* PfoMsgMlpBwd */
  const float* dgi; const float* hid;
  const void* img_wihT; const void* img_w2T;
  float* d_m; float* d_hid;
  int32_t D3, Hm, Md, cap_rows; const int32_t* n_rows;
} pfo_msg_mlp_bwd_desc;
int pfo_debug_msg_mlp_bwd(const pfo_msg_mlp_bwd_desc* f, void* stream);
int pfo_debug_rank1_multi(const pfo_rank1_desc* list, int32_t n, void* stream);
int pfo_debug_sum_slabs(const pfo_sum_slabs_desc* list, int32_t n, void* stream);
/* The launchers' dispatch, asked without launching (additive: the abi version stays).  pfo_debug_gemm_plan /
 * pfo_debug_gemm_tn_group_plan return what pfo_debug_gemm / pfo_debug_gemm_tn_group would do with the same arguments - pure
 * host code, the function the launchers themselves switch on: the form below, or -1 (with the launcher's own message) where
 * the launcher refuses.  Operand layout (a_kmajor / b_kmajor) and `vec` are flags beside the form, not part of it.
 * out[PFO_GEMM_PLAN_INTS] = form, vec (float4 operand loads: the fp32 kernels' flag), grid x, y, z, block, nsplit, chunk
 * (split-K: slabs and k-rows per slab; 1 and 0 where the launch does not split), profiler kind (PFO_PROF_*) of the contraction
 * kernel.  PFO_GEMM_FORM_TN_GROUP: a k-major launch pfo_gemm_launch hands to the grouped split-K launch as one problem -
 * nsplit / chunk are the sizing that made it do so, grid, block are 0 and kind is -1 (the grouped plan of that problem has
 * them).  PFO_GEMM_FORM_MULTI names pfo_gemm_multi_launch's one kernel; it has no query (its only decision is `vec`, which the
 * single-problem query reports per problem). */
#define PFO_GEMM_FORM_F32_128 0     /* gemm_f32_kernel, 128-row tiles                         */
#define PFO_GEMM_FORM_F32_32 1      /* gemm_f32_kernel, 32-row tiles                          */
#define PFO_GEMM_FORM_SKINNY4 2     /* gemm_bx_skinny_kernel<4, 1>: 32 rows x 64 columns      */
#define PFO_GEMM_FORM_SKINNY11 3    /* gemm_bx_skinny_kernel<11, 1>: 32 rows x 176 columns    */
#define PFO_GEMM_FORM_AREG 4        /* gemm_bx_areg_kernel<1>                                 */
#define PFO_GEMM_FORM_AREG8 5       /* gemm_bx_areg8_kernel<1>: eight wavefronts              */
#define PFO_GEMM_FORM_ASTAT 6       /* gemm_bx_astat_kernel: A-stationary                     */
#define PFO_GEMM_FORM_TN_GROUP 7    /* handed to the grouped split-K launch                   */
#define PFO_GEMM_FORM_TN_F32 8      /* gemm_tn_group_kernel                                   */
#define PFO_GEMM_FORM_TN_BX 9       /* gemm_tn_group_bx_kernel<1>: 128-row tiles              */
#define PFO_GEMM_FORM_TN_BX8 10     /* gemm_tn_group_bx_kernel<1, 8>: 256-row tiles           */
#define PFO_GEMM_FORM_MULTI 11      /* gemm_multi_kernel                                      */
#define PFO_GEMM_PLAN_INTS 9
int32_t pfo_debug_gemm_plan(const pfo_gemm_desc* g, int32_t* out /* HOST, PFO_GEMM_PLAN_INTS */);
int32_t pfo_debug_gemm_tn_group_plan(const pfo_tn_desc* probs, int32_t n, int32_t K, int64_t slab_floats,
                                     int32_t* out /* HOST, PFO_GEMM_PLAN_INTS */);

/* debug / test probes of the internal attention interface (csrc/attn.hpp) and of the grouping its run-merged backward
 * consumes (csrc/memory.hpp pfo_seg_build_launch).  As above: the struct mirrors PfoAttn field for field, every call forwards
 * to the internal launcher unchanged, the comments of attn.hpp are the contract, and none of it is part of the drop-in
 * surface (additive: the abi version stays).
 *   pfo_debug_attn_form: the kernel the launcher would take for `desc` - pure host code, the launchers dispatch on the same
 *     function; -1 (with a message) when the descriptor does not pass the launchers' common checks.
 *   pfo_debug_attn_det_parts: slab rows a deterministic backward over N instances writes.
 *   pfo_debug_seg_build: seg_ptr i32[cap_rows + 1], members i32[N], seg_of i32[pfo_debug_seg_of_ints(N)] (optional), scratch
 *     of pfo_debug_seg_scratch_ints(cap_rows) + 2 (cap_rows + 1) + N int32 (the launcher's scan scratch, cursor and unsorted
 *     member list, in this order). */
#define PFO_ATTN_FORM_FWD_RING 0
#define PFO_ATTN_FORM_FWD_REG 1
#define PFO_ATTN_FORM_BWD_RUNS 2
#define PFO_ATTN_FORM_BWD_RING_NONE 3
#define PFO_ATTN_FORM_BWD_RING_DIRECT 4
#define PFO_ATTN_FORM_BWD_NONE 5
#define PFO_ATTN_FORM_BWD_ATOMIC 6
#define PFO_ATTN_FORM_BWD_DET 7
#define PFO_ATTN_FORM_BWD_DIRECT 8
typedef struct pfo_attn_desc {     /* PfoAttn */
  int32_t N, K, D, Ef, H, Cp;
  const float* QK; const int32_t* qk_row; int64_t qk_ld;
  const float* nbr_tab; int64_t nbr_ld; const int32_t* nbr_row; int64_t nbr_row_base;
  int64_t nbr_rows, edge_rows;
  int32_t nbr_relu;
  const int32_t* nbr_ids; const float* edge_feat; const int32_t* eidx; const float* dt; const float* tw; const float* tb;
  float scale, dropout_p;
  uint64_t seed, offset; const uint64_t* offset_dev; const uint8_t* keep_inject;
  float* ctx; float* attw; uint8_t* inv;
  const float* dctx; float* dQK; float* d_nbr; int64_t d_nbr_ld, d_nbr_rep; int32_t d_nbr_nrep;
  double* dtime_part;
  int32_t det; double* dtime_slab; uint8_t* dqk_live;
  const int32_t* members; const int32_t* seg_ptr; const int32_t* n_rows; const int32_t* run_cnt;
} pfo_attn_desc;
int pfo_debug_attn_fwd(const pfo_attn_desc* desc, void* stream);
int pfo_debug_attn_bwd(const pfo_attn_desc* desc, int32_t* n_parts /* HOST, may be NULL */, void* stream);
int64_t pfo_debug_attn_det_parts(int64_t N);
int32_t pfo_debug_attn_form(const pfo_attn_desc* desc, int32_t backward);
int64_t pfo_debug_seg_scratch_ints(int32_t cap_rows);
int64_t pfo_debug_seg_of_ints(int64_t n_members);
int pfo_debug_seg_build(const int32_t* idx, const int32_t* nodes, int32_t N, int32_t cap_rows, const int32_t* key_src,
                        int32_t* seg_ptr, int32_t* members, int32_t* seg_of, int32_t* scratch, int64_t scratch_ints, void* stream);

/* debug / test probes of the memory-side interface (csrc/memory.hpp): one call per internal launcher, the arguments handed on
 * unchanged behind null, count and scratch-size checks.  The comments of memory.hpp are the contract; none of this is part
 * of the drop-in surface (additive: the abi version stays).  Path queries (pure host code, -1 with a message on a bad size):
 *   pfo_debug_msg_store_needs_winner: 1 when a batch of B events takes the atomicMax winner table, 0 for the inline scan.
 *   pfo_debug_gru_gates_bwd_vec: 1 when the launcher takes the float4 kernel for these operands, 0 for the scalar one.
 *   pfo_debug_scan_sweeps: sweeps of 1024 block totals the middle kernel of an n-entry scan takes (2 and more above 2^20).
 *   pfo_debug_fold_parts_rows_in_flight: 8 once a thread of the fold has eight part rows to read at a time, else 1.
 * Sizes: scratch of pfo_debug_touch_compact = pfo_debug_compact_scratch_ints(n_nodes) int32 (its first 2 ceil(n_nodes / 1024)
 * zero when marks_are_zero), of pfo_debug_iscan = n / 1024 + 16 int32, of pfo_debug_fold_parts =
 * pfo_debug_fold_parts_scratch_doubles(n) doubles with 64 int32 tickets (zero before the first use).  pfo_debug_cq_backward takes
 * HOST arrays of n_layers (<= PFO_MAX_LAYERS) device pointers. */
int64_t pfo_debug_compact_scratch_ints(int32_t n_nodes);
int pfo_debug_touch_compact(const int32_t* nodes0, int64_t n0, const int32_t* extra, int64_t n_extra, int32_t n_nodes,
                            int32_t* mark, int32_t* slot, int32_t* touched_ids, int32_t* n_counts, int32_t* scratch,
                            int64_t scratch_ints, int32_t marks_are_zero, int32_t marked, void* stream);
int pfo_debug_pack_remap(const float* msg_table, int32_t M, const float* memory, int32_t D, const uint8_t* has_msg,
                         const int32_t* touched_ids, const int32_t* n_touched, int32_t cap, float* msg_rows, float* h_rows,
                         uint8_t* hm, const int32_t* nodes0, int64_t n0, const int32_t* slot, int32_t* idx0, void* stream);
int32_t pfo_debug_gru_gates_bwd_vec(const float* gates, const float* dgi, const float* dgh, const float* h_rows, int32_t D,
                                    const float* d_h0, int64_t rep_stride, const float* d_extra);
int pfo_debug_gru_gates_bwd(const float* gates, float* dgi, float* dgh, const float* h_rows, const uint8_t* hm,
                            const int32_t* n_touched, int32_t cap, int32_t D, const float* d_h0, int32_t n_rep, int64_t rep_stride,
                            const float* d_extra, int32_t det, void* stream);
int pfo_debug_zero_rows(float* dst, const int32_t* n_rows, int32_t cap_rows, int32_t D, int32_t n_rep, int64_t rep_stride,
                        void* stream);
int pfo_debug_persist(const int32_t* src, const int32_t* dst, int32_t B, const int32_t* slot, const float* upd_mem,
                      const uint8_t* has_msg, const float* msg_time, float* memory, float* last_update, int32_t D,
                      int32_t* winner, void* stream);
int32_t pfo_debug_msg_store_needs_winner(int32_t B);
int pfo_debug_msg_store(const int32_t* src, const int32_t* dst, const double* ts, const int32_t* eidx, int32_t B,
                        const float* memory, const float* last_update, const float* edge_feat, const float* tw, const float* tb,
                        int32_t D, int32_t Ef, float* msg_table, float* msg_time, uint8_t* has_msg, int32_t* winner, void* stream);
int pfo_debug_observe_select(const int32_t* src, const int32_t* dst, int32_t B, const uint8_t* has_msg, int32_t* rep, int32_t base,
                             int32_t* slot, int32_t* touched, int32_t* n_out, void* stream);
int32_t pfo_debug_scan_sweeps(int64_t n);
int pfo_debug_iscan(const int32_t* in, int64_t n, int32_t* out, int32_t* scratch, int64_t scratch_ints, void* stream);
int pfo_debug_mean(const float* src, int64_t n, float* out, void* stream);
int pfo_debug_cq_backward(const float* const* gq, const float* const* Wq, int32_t n_layers, const float* tb, int32_t D,
                          float* const* d_bq, float* const* d_Wq, float* d_tb, float* tb_part, const float* tb_add,
                          const double* dtime, int32_t n_bins, float* d_tw, void* stream);
int64_t pfo_debug_fold_parts_scratch_doubles(int32_t n);
int32_t pfo_debug_fold_parts_rows_in_flight(int32_t n_parts);
int pfo_debug_fold_parts(const double* parts, int32_t n_parts, int32_t n, float* out, int32_t accumulate, double* scratch,
                         int64_t scratch_doubles, int32_t* tickets, double* out64, void* stream);

/* Parameter cache (pfo_tgn_state.pcache): its size, and the call that (re)builds it from state->params on the library's
 * side stream, forked from `stream` and NOT joined back - the next pfo_tgn_forward with pcache_valid = 1 queues its own
 * side-stream work behind it, so the caller's stream never waits for the build itself.  Meant to be called right behind the
 * optimizer's kernel: the build then runs beside the next batch's sampling phase.  Not capturable into a HIP graph
 * (unjoined fork): a captured step passes pcache_valid = 0 instead. */
/* Optimizer step on the library's first side stream, behind a backward that ran with pfo_tgn_batch.defer_join: same
 * arguments and arithmetic as pfo_adam_step_ranges.  Gradients, moments and parameters are then in flight on that stream;
 * pfo_tgn_forward / pfo_tgn_prepare / pfo_tgn_refresh / pfo_tgn_update_state wait for it where they first need them,
 * pfo_tgn_join(stream) makes any other stream wait (no-op when nothing is pending). */
int pfo_tgn_adam_side(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int32_t n_ranges,
                      const int64_t* lo, const int64_t* hi, const int32_t* step, float lr, float beta1, float beta2, float eps);
/* The same step in BUCKETS ordered by first use in the next forward (data-parallel ranks: reduce + step per bucket).
 * bucket 1: the ranges the next pfo_tgn_forward reads on the CALLER's stream (time encoder, GRU, layer 1: everything below
 * pfo_tgn_grad_split) - an event behind this kernel is all that forward's caller's stream waits for; bucket 2: a later bucket of
 * the same step (the top layer's block, whose all-reduce ran beside the backward) - the forward meets it through the side
 * stream's own order (composite weights, fc2 fold); bucket 0: pfo_tgn_adam_side.  Buckets 1 / 2: models with n_layers >= 2. */
int pfo_tgn_adam_side_bucket(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int32_t n_ranges,
                             const int64_t* lo, const int64_t* hi, const int32_t* step, float lr, float beta1, float beta2, float eps,
                             int32_t flags /* bits 0-1: the bucket; bit 2 (4): the kernel also CLEARS the gradient ranges it read -
                                              optimizer.zero_grad() folded in, so that the next pfo_tgn_backward_ev may run with
                                              zero_grad_first = 0 (no clear on its critical path) when the ranges cover the buffer */);
int pfo_tgn_join(void* stream);
/* The library's first side stream (hipStream_t; null on failure): the stream a deferred backward end is left on and
 * pfo_tgn_adam_side runs on.  A data-parallel caller queues its gradient all-reduce THERE, between pfo_tgn_backward
 * (defer_join) and pfo_tgn_adam_side - ordered behind the backward's last launch, in front of the optimizer's kernel, and off the
 * caller's stream, which goes on to the next batch's sampling.  One stream per device, valid for the life of the process. */
void* pfo_tgn_side_stream(void);
int64_t pfo_tgn_pcache_bytes(const pfo_tgn_config* cfg);
int pfo_tgn_refresh(const pfo_tgn_config* cfg, const pfo_tgn_state* state, void* stream);

/* ------------------------------------------------------------------------------------------
 * Live per-kernel timing with HIP events on the launch stream (bench.py roofline numbers).
 * While enabled every launch of the kinds below is bracketed by an event pair; pfo_prof_collect
 * waits for them and returns, per kind, the summed device time [ms], the summed ALGORITHMIC work
 * (FLOP for the GEMM kinds, bytes otherwise - DESIGN.md states the per-unit figures) and the launch count.
 */
#define PFO_PROF_GEMM_NT 0   /* C = A B^T (+bias...)  forward projections                */
#define PFO_PROF_GEMM_NN 1   /* C = A B             backward-data, folded key projection */
#define PFO_PROF_GEMM_TN 2   /* dW = A^T B          weight gradients (split-K + reduce)  */
#define PFO_PROF_GEMM_DEVM 3 /* fp32-MFMA contractions whose extent is a device-side count (work = per-row flops x the count read back) */
#define PFO_PROF_ATTN_FWD 4
#define PFO_PROF_ATTN_BWD 5
#define PFO_PROF_SAMPLER 6
#define PFO_PROF_GEMM_BX 7   /* gemm_bx_areg_kernel and nothing else: every row-major split-contraction launch, device-side row counts included (flops = 2MNK, M read back) */
#define PFO_PROF_GEMM_TN_BX 8 /* grouped weight gradients on the bf16x3 kernel (GEMM kernel only)  */
#define PFO_PROF_GEMM_BX_SKINNY 9 /* the 32-row bf16x3 kernel of the short (layer-2) launches           */
#define PFO_PROF_ATTN_BWD_RUNS 10 /* layer-1 attention backward, run-merged kernel (attn_bwd_runs_kernel)  */
#define PFO_PROF_GRU_FUSED 11 /* gru_fused_kernel: both GRUCell contractions + gates (flops = per-row FLOPs x touched rows read back) */
#define PFO_PROF_GEMM_MULTI 12 /* gemm_multi_kernel: the grouped small fp32 products of the composite-weight builds and their chain-back (FLOP) */
#define PFO_PROF_SEGSUM 13     /* segsum_*_kernel: per-table-row sums of the layer-1 gradient rows (bytes: every member row once + the sums) */
#define PFO_PROF_TN_REDUCE 14  /* tn_group_reduce_kernel: the split-K slabs of a grouped weight-gradient launch folded (bytes: slabs in, matrices out) */
#define PFO_PROF_GRU_GATES_BWD 15 /* gru_gates_bwd_*_kernel: GRU gate backward (bytes: gates, h, d h in; dgi, dgh out) */
#define PFO_PROF_GEMM_TN_BX8 16   /* the same grouped weight gradients on 256-row tiles of eight wavefronts (gemm_tn_group_bx_kernel<1, 8>): a kernel of its own in the traces */
#define PFO_PROF_KINDS 17
/* Milestones: while enabled (pfo_marks_enable(1)) the step's native calls record a timing event on the CALLER's stream at
 * named points of the critical path (sampling done, lazy GRU done, every large launch of every layer ...; callers may add
 * their own with pfo_mark).  pfo_marks_dump waits for them and writes one line per consecutive pair "from -> to  mean_us  n"
 * in first-seen order: the segments of the caller's stream as the GPU ran them, WITHOUT a tracer slowing the host down.
 * ~1 us per mark; off by default. */
int pfo_marks_enable(int32_t on);
int pfo_mark(const char* name /* static string */, void* stream);
int64_t pfo_marks_dump(char* out, int64_t cap); /* HOST buffer; returns the bytes written (0-terminated), clears the records */
int pfo_prof_enable(int32_t on);
int pfo_prof_collect(double* ms, double* work, int64_t* count); /* HOST arrays of PFO_PROF_KINDS entries */
/* Shader clock under the product kernels [GHz]: the first wavefront of three large kernels stamps the shader cycle counter
 * against the constant 100 MHz counter on every launch (two scalar reads, two atomics per launch).  out[0] attention forward
 * (ring form), out[1] run-merged attention backward, out[2] grouped weight-gradient kernel; 0 where the kernel has not run since
 * the last reset.  The peaks of MI355X_MICROARCH.md are priced at 2.4 GHz: bench.py prints both. */
#define PFO_CLOCK_KERNELS 3
int pfo_shader_clock(double* ghz_out /* HOST, PFO_CLOCK_KERNELS entries */, int32_t reset);

#ifdef __cplusplus
}
#endif
#endif /* PFOTGN_H */
