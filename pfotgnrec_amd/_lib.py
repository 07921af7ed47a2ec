"""ctypes binding of libpfotgn.so (the C ABI declared in include/pfotgn.h).

There is no CPU fallback: if the library is missing, loading raises; if no HIP device is present,
every compute entry raises ``RuntimeError`` before anything is launched.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PFOTGN_LIB", os.path.join(_HERE, "lib", "libpfotgn.so"))   # override: kernel A/B builds

c_i32p = C.c_void_p   # device pointers travel as integers (tensor.data_ptr())
_VP = C.c_void_p

MAX_LAYERS = 4
RECOMMEND_MAX_ITEMS = 65536     # PFO_RECOMMEND_MAX_ITEMS
RECOMMEND_MV_MAX_ITEMS = 2048   # PFO_RECOMMEND_MV_MAX_ITEMS
RECOMMEND_MV_WIDE_MAX_ITEMS = 65536   # PFO_RECOMMEND_MV_WIDE_MAX_ITEMS
RECOMMEND_LIST_MAX_WIDTH = 256  # PFO_RECOMMEND_LIST_MAX_WIDTH
RECOMMEND_HELD_MAX_WIDTH = 256  # PFO_RECOMMEND_HELD_MAX_WIDTH
HISTORY_MAX_WIDTH = 256         # PFO_HISTORY_MAX_WIDTH
EXPLAIN_MAX_WIDTH = 256         # PFO_EXPLAIN_MAX_WIDTH
MAX_NEIGHBORS = 64              # PFO_MAX_NEIGHBORS
DEFAULT_NEIGHBORS = 20          # n_neighbors of the entry points (compute_temporal_embeddings) when model and caller name none
EVAL_RANK_NONE = (1 << 31) - 1  # PFO_EVAL_RANK_NONE: the positive is not ranked
ADAM_MAX_RANGES = 16            # PFO_ADAM_MAX_RANGES
GRAD_NORM_PARTS = 256           # PFO_GRAD_NORM_PARTS


class TgnConfig(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("n_edges_p1", C.c_int32), ("D", C.c_int32), ("Ef", C.c_int32),
                ("n_layers", C.c_int32), ("n_heads", C.c_int32), ("use_memory", C.c_int32), ("max_roots", C.c_int32),
                ("max_neighbors", C.c_int32), ("max_batch", C.c_int32), ("msg_dim", C.c_int32), ("msg_hidden", C.c_int32)]


class TgnLayerLayout(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("wq", "wk", "wv", "b_in", "wo", "bo", "w1", "b1", "w2", "b2")]


class TgnLayout(C.Structure):
    _fields_ = [("time_w", C.c_int64), ("time_b", C.c_int64), ("gru_w_ih", C.c_int64), ("gru_w_hh", C.c_int64),
                ("gru_b_ih", C.c_int64), ("gru_b_hh", C.c_int64), ("layer", TgnLayerLayout * MAX_LAYERS),
                ("total", C.c_int64), ("mlp_w1", C.c_int64), ("mlp_b1", C.c_int64), ("mlp_w2", C.c_int64), ("mlp_b2", C.c_int64)]


class TgnState(C.Structure):
    _fields_ = [(n, _VP) for n in ("indptr", "adj_nbr", "adj_eidx", "adj_ts", "node_feat", "edge_feat", "memory",
                                   "last_update", "msg_table", "msg_time", "has_msg", "params", "pcache")] + [("pcache_valid", C.c_int32)]


class TgnBatch(C.Structure):
    _fields_ = [("roots", _VP), ("root_ts", _VP), ("R", C.c_int32), ("K", C.c_int32), ("uniform", C.c_int32),
                ("draws", C.POINTER(_VP)), ("seed", C.c_uint64), ("offset", C.c_uint64), ("dropout_p", C.c_float),
                ("training", C.c_int32), ("extra_nodes", _VP), ("n_extra", C.c_int32), ("offset_dev", _VP),
                ("deterministic", C.c_int32), ("prepared", C.c_int32),
                ("upd_src", _VP), ("upd_dst", _VP), ("upd_ts", _VP), ("upd_eidx", _VP), ("upd_B", C.c_int32),
                ("dropout_keep", C.POINTER(_VP)), ("mid_event", _VP), ("defer_join", C.c_int32), ("seg_in_forward", C.c_int32), ("mid_event_late", C.c_int32)]


class TgnDebug(C.Structure):
    _fields_ = [(n, _VP) for n in ("n_touched", "touched_ids", "h0_table", "slot", "n_core", "l1_ctx", "l1_dh1", "l1_dW1ovT",
                                   "gru_dgi", "gru_msg_rows")] + [("Cp", C.c_int32), ("mlp_hid", _VP), ("mlp_out", _VP)]


# debug / test probes of the internal contraction interface (csrc/gemm.hpp through csrc/probe.hip); the package never calls them
_FP = C.c_void_p


class GemmDesc(C.Structure):
    _fields_ = [("A", _FP * 2), ("lda", C.c_int64 * 2), ("a_idx", _FP * 2), ("B", _FP * 2), ("ldb", C.c_int64 * 2), ("b_idx", _FP),
                ("K", C.c_int32 * 2), ("C", _FP), ("ldc", C.c_int64), ("bias", _FP), ("row_scale", _FP), ("rs_ld", C.c_int64),
                ("row_zero", _FP), ("relu_src", _FP), ("relu_ld", C.c_int64), ("add_src", _FP), ("add_ld", C.c_int64),
                ("add_idx", _FP), ("M", C.c_int32), ("N", C.c_int32), ("m_dev", _FP), ("relu", C.c_int32),
                ("accumulate", C.c_int32), ("a_kmajor", C.c_int32), ("b_kmajor", C.c_int32), ("batch", C.c_int32),
                ("a_bs", C.c_int64 * 2), ("b_bs", C.c_int64 * 2), ("c_bs", C.c_int64), ("bias_bs", C.c_int64), ("rs_bs", C.c_int64),
                ("slabs", _FP), ("slab_floats", C.c_int64), ("b_img", _FP), ("b_img2", _FP), ("bx_force", C.c_int32)]


class TnDesc(C.Structure):
    _fields_ = [("A", _FP), ("lda", C.c_int64), ("B", _FP), ("ldb", C.c_int64), ("b_idx", _FP), ("M", C.c_int32), ("N", C.c_int32),
                ("C", _FP), ("ldc", C.c_int64), ("c_accumulate", C.c_int32), ("bias_out", _FP), ("bias_accumulate", C.c_int32)]


class BimgDesc(C.Structure):
    _fields_ = [("src", _FP), ("ld", C.c_int64), ("N", C.c_int32), ("K", C.c_int32), ("trans", C.c_int32), ("dst", _FP),
                ("row0", C.c_int32), ("rows_total", C.c_int32), ("last", C.c_int32), ("gate", C.c_int32), ("gate_D", C.c_int32)]


class GruDesc(C.Structure):
    _fields_ = [("msg_rows", _FP), ("K_msg", C.c_int32), ("h_rows", _FP), ("img_ih", _FP), ("img_hh", _FP), ("b_ih", _FP),
                ("b_hh", _FP), ("hm", _FP), ("touched", _FP), ("node_feat", _FP), ("upd_mem", _FP), ("h0_tab", _FP), ("gates", _FP),
                ("D", C.c_int32), ("cap_rows", C.c_int32), ("n_rows", _FP), ("gather", C.c_int32)]


class MsgMlpDesc(C.Structure):
    _fields_ = [("raw", _FP), ("ld_raw", C.c_int64), ("touched", _FP), ("hm", _FP), ("img_w1", _FP), ("img_w2", _FP), ("b1", _FP),
                ("b2", _FP), ("hid", _FP), ("msg_out", _FP), ("Mr", C.c_int32), ("Hm", C.c_int32), ("Md", C.c_int32),
                ("cap_rows", C.c_int32), ("n_rows", _FP)]


class MsgMlpBwdDesc(C.Structure):
    _fields_ = [("dgi", _FP), ("hid", _FP), ("img_wihT", _FP), ("img_w2T", _FP), ("d_m", _FP), ("d_hid", _FP), ("D3", C.c_int32),
                ("Hm", C.c_int32), ("Md", C.c_int32), ("cap_rows", C.c_int32), ("n_rows", _FP)]


class Rank1Desc(C.Structure):
    _fields_ = [("u", _FP), ("ldu", C.c_int64), ("v", _FP), ("ldv", C.c_int64), ("M", C.c_int32), ("N", C.c_int32), ("out", _FP),
                ("ldo", C.c_int64), ("reps", C.c_int32), ("u_rs", C.c_int64), ("v_rs", C.c_int64)]


class SumSlabsDesc(C.Structure):
    _fields_ = [("dst", _FP), ("src", _FP), ("stride", C.c_int64), ("count", C.c_int64), ("n_slabs", C.c_int32),
                ("accumulate", C.c_int32)]


# ... and of the internal attention interface (csrc/attn.hpp)
class AttnDesc(C.Structure):
    _fields_ = [("N", C.c_int32), ("K", C.c_int32), ("D", C.c_int32), ("Ef", C.c_int32), ("H", C.c_int32), ("Cp", C.c_int32),
                ("QK", _FP), ("qk_row", _FP), ("qk_ld", C.c_int64),
                ("nbr_tab", _FP), ("nbr_ld", C.c_int64), ("nbr_row", _FP), ("nbr_row_base", C.c_int64),
                ("nbr_rows", C.c_int64), ("edge_rows", C.c_int64), ("nbr_relu", C.c_int32),
                ("nbr_ids", _FP), ("edge_feat", _FP), ("eidx", _FP), ("dt", _FP), ("tw", _FP), ("tb", _FP),
                ("scale", C.c_float), ("dropout_p", C.c_float), ("seed", C.c_uint64), ("offset", C.c_uint64), ("offset_dev", _FP),
                ("keep_inject", _FP), ("ctx", _FP), ("attw", _FP), ("inv", _FP),
                ("dctx", _FP), ("dQK", _FP), ("d_nbr", _FP), ("d_nbr_ld", C.c_int64), ("d_nbr_rep", C.c_int64),
                ("d_nbr_nrep", C.c_int32), ("dtime_part", _FP), ("det", C.c_int32), ("dtime_slab", _FP), ("dqk_live", _FP),
                ("members", _FP), ("seg_ptr", _FP), ("n_rows", _FP), ("run_cnt", _FP)]


# PFO_GEMM_FORM_* and the fields of a plan query's out[PFO_GEMM_PLAN_INTS]
GEMM_FORMS = ["f32_128", "f32_32", "skinny4", "skinny11", "areg", "areg8", "astat", "tn_group", "tn_f32", "tn_bx", "tn_bx8", "multi"]
GEMM_PLAN_FIELDS = ["form", "vec", "grid_x", "grid_y", "grid_z", "block", "nsplit", "chunk", "kind"]
ATTN_FORMS = ["fwd_ring", "fwd_reg", "bwd_runs", "bwd_ring_none", "bwd_ring_direct", "bwd_none", "bwd_atomic", "bwd_det", "bwd_direct"]


# name -> (restype, argtypes); every symbol of include/pfotgn.h
PROTOTYPES = {
    "pfo_abi_version": (C.c_int, []),
    "pfo_last_error": (C.c_char_p, []),
    "pfo_tnbr_sample": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, _VP,
                                  C.c_uint64, C.c_uint64, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "pfo_neg_draw": (C.c_int, [_VP, C.c_int32, _VP, _VP, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_uint64,
                               C.c_uint64, _VP, _VP]),
    "pfo_neg_draw_dev": (C.c_int, [_VP, C.c_int32, _VP, _VP, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_uint64,
                                   C.c_uint64, _VP, _VP, _VP]),
    "pfo_mv_select": (C.c_int, [_VP, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, C.c_int32, _VP, _VP, C.c_int32,
                                C.c_int64, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_int32, _VP, _VP, _VP,
                                _VP, _VP]),
    "pfo_time_encode": (C.c_int, [_VP, C.c_int64, _VP, _VP, C.c_int32, _VP, _VP]),
    "pfo_segment_sum": (C.c_int, [_VP, C.c_int32, _VP, C.c_int32, _VP, _VP, _VP, C.c_int64, _VP, C.c_int32, C.c_int32, _VP, _VP,
                                  _VP]),
    "pfo_attn_dropout_mask": (C.c_int, [C.c_uint64, C.c_uint64, C.c_int64, C.c_int32, C.c_int32, C.c_float, _VP, _VP]),
    "pfo_gemm_f32": (C.c_int, [_VP, C.c_int64, C.c_int32, _VP, C.c_int64, C.c_int32, _VP, C.c_int64, _VP, C.c_int32,
                               C.c_int32, C.c_int32, C.c_int32, _VP, C.c_int64, _VP]),
    "pfo_gemm_bf16x3_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "pfo_gemm_bf16x3": (C.c_int, [_VP, C.c_int64, _VP, C.c_int64, C.c_int32, _VP, C.c_int64, _VP, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_int32, _VP, C.c_int64, _VP]),
    "pfo_roots_assemble": (C.c_int, [_VP, _VP, _VP, C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int32,
                                     _VP, _VP, _VP]),
    "pfo_bpr_loss": (C.c_int, [_VP, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_float, _VP,
                               _VP, _VP, _VP]),
    "pfo_bpr_loss_fused": (C.c_int, [_VP, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_float, _VP,
                                     _VP, _VP, _VP, _VP]),
    "pfo_bpr_loss_parts": (C.c_int, [_VP, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_float, _VP,
                                     _VP, _VP]),
    "pfo_rank_metrics": (C.c_int, [_VP, C.c_int64, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP]),
    "pfo_eval_metrics": (C.c_int, [_VP, C.c_int64, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, C.c_int32, _VP, _VP, C.c_int32,
                                   C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "pfo_eval_metrics_mv": (C.c_int, [_VP, C.c_int64, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, C.c_int32, _VP, _VP, C.c_int32,
                                      C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, _VP, _VP, _VP, _VP, _VP, _VP,
                                      _VP, C.c_int32, C.c_int32, C.c_int32, _VP, C.c_double, C.c_double, C.c_int32, _VP, _VP, _VP, _VP,
                                      _VP, _VP]),
    "pfo_list_metrics": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int32, C.POINTER(C.c_int32), C.c_int32, _VP, _VP, C.c_int32,
                                   C.c_int32, _VP, _VP, C.c_int32, C.c_int32, _VP, _VP, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                   C.c_int64, _VP, _VP, _VP, _VP, _VP]),
    "pfo_recommend_topk": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, C.c_int32, _VP, C.c_int32,
                                     _VP, _VP, _VP, _VP]),
    "pfo_recommend_mv_topk": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, C.c_int32, _VP,
                                        _VP, _VP, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, _VP, C.c_int32, C.c_double, C.c_double,
                                        C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "pfo_recommend_mv_wide_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int32]),
    "pfo_recommend_mv_topk_wide": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, C.c_int32, _VP,
                                             _VP, _VP, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, _VP, C.c_int32, C.c_double, C.c_double,
                                             C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_int64, _VP]),
    "pfo_recommend_basket_topk": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, C.c_int32, _VP,
                                            _VP, _VP, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, _VP, C.c_int32, C.c_double,
                                            C.c_double, C.c_int32, _VP, _VP, _VP, _VP, _VP]),
    # the capped forms: (cand_group, group_cap) behind item_ok
    "pfo_recommend_topk_capped": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, C.c_int32, _VP, _VP,
                                            C.c_int32, C.c_int32, _VP, _VP, _VP, _VP]),
    "pfo_recommend_mv_topk_capped": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, C.c_int32, _VP, _VP,
                                               C.c_int32, _VP, _VP, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, _VP, C.c_int32, C.c_double,
                                               C.c_double, C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "pfo_recommend_basket_topk_capped": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, C.c_int32, _VP,
                                                   _VP, C.c_int32, _VP, _VP, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, _VP, C.c_int32,
                                                   C.c_double, C.c_double, C.c_int32, _VP, _VP, _VP, _VP, _VP]),
    # the _held forms: (held_group, held_len, held_stride) behind group_cap
    "pfo_recommend_topk_capped_held": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, C.c_int32, _VP, _VP,
                                                 C.c_int32, _VP, _VP, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP]),
    "pfo_recommend_mv_topk_capped_held": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, C.c_int32, _VP,
                                                    _VP, C.c_int32, _VP, _VP, C.c_int32, _VP, _VP, C.c_int32, C.c_int32, C.c_int32, _VP,
                                                    _VP, _VP, C.c_int32, C.c_double, C.c_double, C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP,
                                                    _VP, _VP]),
    "pfo_recommend_basket_topk_capped_held": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, C.c_int32,
                                                        _VP, _VP, C.c_int32, _VP, _VP, C.c_int32, _VP, _VP, C.c_int32, C.c_int32,
                                                        C.c_int32, _VP, _VP, _VP, C.c_int32, C.c_double, C.c_double, C.c_int32, _VP, _VP,
                                                        _VP, _VP, _VP]),
    "pfo_recommend_list_topk": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, C.c_int32, _VP,
                                          C.c_int32, _VP, _VP, _VP, _VP, _VP]),
    "pfo_recommend_list_mv_topk": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, C.c_int32, _VP,
                                             _VP, _VP, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, _VP, C.c_int32, C.c_double, C.c_double,
                                             C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    # the weighted forms: port_w behind port_len
    "pfo_recommend_mv_topk_weighted": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, C.c_int32, _VP,
                                                 _VP, _VP, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, C.c_int32, C.c_double,
                                                 C.c_double, C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "pfo_recommend_mv_topk_wide_weighted": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, C.c_int32, _VP,
                                                      _VP, _VP, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, C.c_int32, C.c_double,
                                                      C.c_double, C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_int64, _VP]),
    "pfo_recommend_list_mv_topk_weighted": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, C.c_int32, _VP,
                                                      _VP, _VP, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, C.c_int32, C.c_double,
                                                      C.c_double, C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "pfo_adam_step": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32,
                                _VP]),
    "pfo_csr_build_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int64]),
    "pfo_csr_build": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, C.c_int64, _VP, _VP, _VP, _VP, _VP, C.c_int64, _VP]),
    "pfo_debug_csr_build_plan": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_int32)]),
    "pfo_csr_append": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, _VP, _VP, _VP, _VP, C.c_int64, _VP, _VP, _VP, _VP, _VP]),
    "pfo_csr_expire_scratch_bytes": (C.c_int64, [C.c_int64]),
    "pfo_csr_expire_plan": (C.c_int, [_VP, _VP, C.c_int64, C.c_double, _VP, _VP, _VP, C.c_int64, _VP]),
    "pfo_csr_expire_copy": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, _VP, _VP, C.c_int64, _VP, _VP, _VP, _VP]),
    "pfo_adam_step_ranges": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                       C.POINTER(C.c_int32), C.c_float, C.c_float, C.c_float, C.c_float, _VP]),
    "pfo_adam_step_ranges_dev": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                           C.POINTER(C.c_int32), _VP, C.c_float, C.c_float, C.c_float, C.c_float, _VP]),
    "pfo_grad_sumsq_ranges": (C.c_int, [_VP, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _VP, C.c_int32, _VP]),
    "pfo_grad_prestep_ranges": (C.c_int, [_VP, _VP, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _VP, C.c_float, C.c_float,
                                          _VP, _VP]),
    "pfo_tgn_param_layout": (C.c_int, [C.POINTER(TgnConfig), C.POINTER(TgnLayout)]),
    "pfo_tgn_workspace_bytes": (C.c_int64, [C.POINTER(TgnConfig)]),
    "pfo_tgn_adam_side": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                    C.POINTER(C.c_int32), C.c_float, C.c_float, C.c_float, C.c_float]),
    "pfo_tgn_adam_side_bucket": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                          C.POINTER(C.c_int32), C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32]),
    "pfo_tgn_side_stream": (_VP, []),
    "pfo_tgn_join": (C.c_int, [_VP]),
    "pfo_tgn_pcache_bytes": (C.c_int64, [C.POINTER(TgnConfig)]),
    "pfo_tgn_refresh": (C.c_int, [C.POINTER(TgnConfig), C.POINTER(TgnState), _VP]),
    "pfo_tgn_forward": (C.c_int, [C.POINTER(TgnConfig), C.POINTER(TgnState), C.POINTER(TgnBatch), _VP, _VP, _VP]),
    "pfo_tgn_prepare": (C.c_int, [C.POINTER(TgnConfig), C.POINTER(TgnState), C.POINTER(TgnBatch), _VP, _VP]),
    "pfo_tgn_backward": (C.c_int, [C.POINTER(TgnConfig), C.POINTER(TgnState), C.POINTER(TgnBatch), _VP, _VP, _VP, _VP]),
    "pfo_tgn_backward_ev": (C.c_int, [C.POINTER(TgnConfig), C.POINTER(TgnState), C.POINTER(TgnBatch), _VP, _VP, _VP, C.c_int32,
                                      _VP, _VP, C.c_int64, _VP, _VP]),
    "pfo_tgn_grad_split": (C.c_int, [C.POINTER(TgnConfig), C.POINTER(C.c_int64)]),
    "pfo_tgn_update_state": (C.c_int, [C.POINTER(TgnConfig), C.POINTER(TgnState), _VP, _VP, _VP, _VP, C.c_int32, _VP,
                                       _VP]),
    "pfo_tgn_observe_workspace_bytes": (C.c_int64, [C.POINTER(TgnConfig), C.c_int32]),
    "pfo_tgn_observe": (C.c_int, [C.POINTER(TgnConfig), C.POINTER(TgnState), _VP, _VP, _VP, _VP, C.c_int64, C.c_int32, _VP,
                                  C.c_int64, _VP]),
    "pfo_edge_rows_append": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int32, _VP, C.c_int64, C.c_int64, _VP]),
    "pfo_edge_rows_mark": (C.c_int, [_VP, _VP, C.c_int64, C.c_double, C.c_int64, _VP, _VP]),
    "pfo_edge_rows_plan_scratch_bytes": (C.c_int64, [C.c_int64]),
    "pfo_edge_rows_plan": (C.c_int, [_VP, C.c_int64, _VP, _VP, _VP, C.c_int64, _VP]),
    "pfo_edge_rows_compact": (C.c_int, [_VP, C.c_int64, C.c_int64, C.c_int32, _VP, _VP, _VP]),
    "pfo_eidx_remap": (C.c_int, [_VP, C.c_int64, _VP, C.c_int64, _VP]),
    "pfo_nodes_flag": (C.c_int, [_VP, C.c_int64, C.c_int64, _VP, _VP]),
    "pfo_csr_forget_scratch_bytes": (C.c_int64, [C.c_int64, C.c_int64]),
    "pfo_csr_forget_plan": (C.c_int, [_VP, _VP, C.c_int64, C.c_int64, _VP, _VP, _VP, _VP, _VP, C.c_int64, _VP]),
    "pfo_csr_forget_copy": (C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, _VP, C.c_int64, _VP, _VP, _VP, _VP]),
    "pfo_edge_rows_mark_nodes": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int64, _VP, C.c_int64, _VP, _VP]),
    "pfo_node_rows_reset": (C.c_int, [_VP, C.c_int64, _VP, C.c_int32, _VP, _VP, C.c_int32, _VP, _VP, _VP, C.c_int32, _VP, C.c_int32,
                                      _VP, _VP, _VP]),
    "pfo_holdings_store_scratch_bytes": (C.c_int64, [C.c_int64, C.c_int64]),
    "pfo_holdings_store": (C.c_int, [_VP, _VP, _VP, C.c_int32, _VP, C.c_int64, _VP, _VP, _VP, C.c_int64, C.c_int32, _VP, C.c_int64,
                                     _VP]),
    "pfo_holdings_gather": (C.c_int, [_VP, C.c_int64, _VP, _VP, C.c_int64, C.c_int32, _VP, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP,
                                      _VP]),
    "pfo_holdings_apply_scratch_bytes": (C.c_int64, [C.c_int64, C.c_int64]),
    "pfo_holdings_apply": (C.c_int, [_VP, _VP, _VP, _VP, _VP, C.c_int64, _VP, _VP, _VP, _VP, C.c_int64, C.c_int32, _VP, _VP, C.c_int64,
                                     _VP]),
    "pfo_holdings_gather_weights": (C.c_int, [_VP, C.c_int64, _VP, _VP, _VP, C.c_int64, C.c_int32, _VP, C.c_int64, C.c_int32, _VP, _VP]),
    "pfo_history_gather": (C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int64, _VP, C.c_int32, _VP, C.c_int32,
                                     _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "pfo_returns_scatter_scratch_bytes": (C.c_int64, [C.c_int64]),
    "pfo_returns_scatter_closes": (C.c_int, [_VP, _VP, C.c_int64, C.c_int64, _VP, C.c_int64, _VP]),
    "pfo_returns_append_day": (C.c_int, [_VP, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, _VP, C.c_int64, _VP, _VP,
                                         _VP, C.c_int64, _VP, _VP]),
    "pfo_day_lookup": (C.c_int, [_VP, C.c_int64, _VP, C.c_int32, C.c_int32, C.c_int32, C.c_double, _VP, _VP]),
    "pfo_tgn_debug_views": (C.c_int,[C.POINTER(TgnConfig), _VP, C.POINTER(TgnDebug)]),
    "pfo_tgn_explain": (C.c_int, [C.POINTER(TgnConfig), _VP, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP,
                                  _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "pfo_debug_gemm": (C.c_int, [C.POINTER(GemmDesc), _VP]),
    "pfo_debug_gemm_multi": (C.c_int, [C.POINTER(GemmDesc), C.c_int32, _VP]),
    "pfo_debug_gemm_tn_group": (C.c_int, [C.POINTER(TnDesc), C.c_int32, C.c_int32, _VP, _VP, C.c_int64, _VP]),
    "pfo_debug_gemm_plan": (C.c_int32, [C.POINTER(GemmDesc), C.POINTER(C.c_int32)]),
    "pfo_debug_gemm_tn_group_plan": (C.c_int32, [C.POINTER(TnDesc), C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_int32)]),
    "pfo_debug_bimg_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "pfo_debug_gru_img_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "pfo_debug_bimg": (C.c_int, [C.POINTER(BimgDesc), C.c_int32, _VP]),
    "pfo_debug_gru_fused": (C.c_int, [C.POINTER(GruDesc), _VP]),
    "pfo_debug_msg_mlp_fwd": (C.c_int, [C.POINTER(MsgMlpDesc), _VP]),
    "pfo_debug_msg_mlp_bwd": (C.c_int, [C.POINTER(MsgMlpBwdDesc), _VP]),
    "pfo_debug_rank1_multi": (C.c_int, [C.POINTER(Rank1Desc), C.c_int32, _VP]),
    "pfo_debug_sum_slabs": (C.c_int, [C.POINTER(SumSlabsDesc), C.c_int32, _VP]),
    "pfo_debug_attn_fwd": (C.c_int, [C.POINTER(AttnDesc), _VP]),
    "pfo_debug_attn_bwd": (C.c_int, [C.POINTER(AttnDesc), C.POINTER(C.c_int32), _VP]),
    "pfo_debug_attn_det_parts": (C.c_int64, [C.c_int64]),
    "pfo_debug_attn_form": (C.c_int32, [C.POINTER(AttnDesc), C.c_int32]),
    "pfo_debug_seg_scratch_ints": (C.c_int64, [C.c_int32]),
    "pfo_debug_seg_of_ints": (C.c_int64, [C.c_int64]),
    "pfo_debug_seg_build": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, _VP, C.c_int64, _VP]),
    # ... and of the memory-side interface (csrc/memory.hpp), one per launcher
    "pfo_debug_compact_scratch_ints": (C.c_int64, [C.c_int32]),
    "pfo_debug_touch_compact": (C.c_int, [_VP, C.c_int64, _VP, C.c_int64, C.c_int32, _VP, _VP, _VP, _VP, _VP, C.c_int64, C.c_int32,
                                          C.c_int32, _VP]),
    "pfo_debug_pack_remap": (C.c_int, [_VP, C.c_int32, _VP, C.c_int32, _VP, _VP, _VP, C.c_int32, _VP, _VP, _VP, _VP, C.c_int64, _VP,
                                       _VP, _VP]),
    "pfo_debug_gru_gates_bwd_vec": (C.c_int32, [_VP, _VP, _VP, _VP, C.c_int32, _VP, C.c_int64, _VP]),
    "pfo_debug_gru_gates_bwd": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, C.c_int32, C.c_int32, _VP, C.c_int32, C.c_int64, _VP,
                                          C.c_int32, _VP]),
    "pfo_debug_zero_rows": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.c_int32, C.c_int64, _VP]),
    "pfo_debug_persist": (C.c_int, [_VP, _VP, C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP, C.c_int32, _VP, _VP]),
    "pfo_debug_msg_store_needs_winner": (C.c_int32, [C.c_int32]),
    "pfo_debug_msg_store": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int32, _VP, _VP, _VP, _VP, _VP, C.c_int32, C.c_int32, _VP, _VP, _VP,
                                      _VP, _VP]),
    "pfo_debug_observe_select": (C.c_int, [_VP, _VP, C.c_int32, _VP, _VP, C.c_int32, _VP, _VP, _VP, _VP]),
    "pfo_debug_scan_sweeps": (C.c_int32, [C.c_int64]),
    "pfo_debug_iscan": (C.c_int, [_VP, C.c_int64, _VP, _VP, C.c_int64, _VP]),
    "pfo_debug_mean": (C.c_int, [_VP, C.c_int64, _VP, _VP]),
    "pfo_debug_cq_backward": (C.c_int, [C.POINTER(_VP), C.POINTER(_VP), C.c_int32, _VP, C.c_int32, C.POINTER(_VP), C.POINTER(_VP),
                                        _VP, _VP, _VP, _VP, C.c_int32, _VP, _VP]),
    "pfo_debug_fold_parts_scratch_doubles": (C.c_int64, [C.c_int32]),
    "pfo_debug_fold_parts_rows_in_flight": (C.c_int32, [C.c_int32]),
    "pfo_debug_fold_parts": (C.c_int, [_VP, C.c_int32, C.c_int32, _VP, C.c_int32, _VP, C.c_int64, _VP, _VP, _VP]),
    "pfo_prof_enable": (C.c_int, [C.c_int32]),
    "pfo_marks_enable": (C.c_int, [C.c_int32]),
    "pfo_mark": (C.c_int, [C.c_char_p, _VP]),
    "pfo_marks_dump": (C.c_int64, [C.c_char_p, C.c_int64]),
    "pfo_prof_collect": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "pfo_shader_clock": (C.c_int, [C.POINTER(C.c_double), C.c_int32]),
}

PROF_KINDS = ["gemm_nt", "gemm_nn", "gemm_tn", "gemm_devm", "attn_fwd", "attn_bwd", "sampler", "gemm_bx", "gemm_tn_bx", "gemm_bx_skinny",
              "attn_bwd_runs", "gru_fused", "gemm_multi", "segsum", "tn_reduce", "gru_gates_bwd", "gemm_tn_bx8"]


_MARK_NAMES = {}


def mark(name):
    """A milestone on the current stream (no-op unless ``marks_enable(True)``); the C side keeps the pointer, so the bytes
    object of every name is kept alive here."""
    b = _MARK_NAMES.get(name)
    if b is None:
        b = _MARK_NAMES[name] = C.c_char_p(name.encode())
    load().pfo_mark(b, stream_ptr())


def marks_enable(on):
    call("pfo_marks_enable", 1 if on else 0)


def marks_dump():
    buf = C.create_string_buffer(1 << 16)
    load().pfo_marks_dump(buf, len(buf))
    return buf.value.decode()


_PROF_ON = [False]


def prof_enable(on):
    _PROF_ON[0] = bool(on)
    call("pfo_prof_enable", 1 if on else 0)


def prof_is_on():
    return _PROF_ON[0]


CLOCK_KERNELS = ["attn_fwd", "attn_bwd_runs", "gemm_tn_bx"]


def shader_clock(reset=False):
    """GHz the first wavefront of the three stamped kernels ran at since the last reset (0.0: not launched)."""
    out = (C.c_double * len(CLOCK_KERNELS))()
    call("pfo_shader_clock", out, 1 if reset else 0)
    return {k: out[i] for i, k in enumerate(CLOCK_KERNELS)}


def prof_collect():
    n = len(PROF_KINDS)
    ms, work, cnt = (C.c_double * n)(), (C.c_double * n)(), (C.c_int64 * n)()
    call("pfo_prof_collect", ms, work, cnt)
    return {k: dict(ms=ms[i], work=work[i], count=cnt[i]) for i, k in enumerate(PROF_KINDS)}

_lib = None


class PfoError(RuntimeError):
    pass


def load():
    """Loads the shared library (raises if it has not been built: run ``python -m pfotgnrec_amd.build``)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PfoError("libpfotgn.so not found at %s - build it with `python -m pfotgnrec_amd.build` "
                           "(there is no CPU fallback)" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def call(name, *args):
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise PfoError("%s failed (%d): %s" % (name, rc, lib.pfo_last_error().decode()))


def byte_count(name, *args):
    """A ``*_bytes`` query of the library: the count it returns, or ``PfoError`` with its message when that is negative."""
    lib = load()
    n = getattr(lib, name)(*args)
    if n < 0:
        raise PfoError("%s: %s" % (name, lib.pfo_last_error().decode()))
    return n


def gemm_plan(name, *args):
    """A ``pfo_debug_gemm*_plan`` query: its ``out`` array as a dict, ``form`` by its name in ``GEMM_FORMS`` and ``kind`` by its
    name in ``PROF_KINDS``; ``PfoError`` with the launcher's message where the launcher would refuse the arguments."""
    lib = load()
    out = (C.c_int32 * len(GEMM_PLAN_FIELDS))()
    if getattr(lib, name)(*args, out) < 0:
        raise PfoError("%s: %s" % (name, lib.pfo_last_error().decode()))
    plan = dict(zip(GEMM_PLAN_FIELDS, out))
    plan["form"] = GEMM_FORMS[plan["form"]]
    plan["kind"] = PROF_KINDS[plan["kind"]] if plan["kind"] >= 0 else None
    return plan


def csr_build_plan(E, n_nodes):
    """``pfo_debug_csr_build_plan``: ``(tiles, owner passes, histogram-scan sweeps)`` of a ``pfo_csr_build`` over these sizes;
    ``PfoError`` with the message where the build would refuse them."""
    out = (C.c_int32 * 3)()
    call("pfo_debug_csr_build_plan", int(E), int(n_nodes), out)
    return tuple(out)


_GPU_SEEN = [False]


def require_gpu(device=None):
    # (torch.cuda.is_available() reads the environment on every call: ~3 us, a dozen times per step - asked once)
    if not _GPU_SEEN[0]:
        import torch
        if not torch.cuda.is_available():
            raise PfoError("a HIP device (MI355X) is required: the hot path has no CPU implementation")
        _GPU_SEEN[0] = True
    if device is not None:
        t = getattr(device, "type", None)
        if t is None:
            import torch
            t = torch.device(device).type
        if t != "cuda":
            raise PfoError("tensors must live on a HIP device, got %s" % device)


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


# torch.cuda.current_stream() builds a Stream object through several Python layers (~8 us); the step asks for the current
# stream's handle a dozen times.  The raw handle comes from one C call; Stream OBJECTS (for Event.record / Stream.wait_event)
# are kept per handle - torch's streams live in a pool and are never destroyed, an external stream is its handle.
_RAW = [None, None]
_STREAM_OBJECTS = {}


def _raw_fns():
    import torch
    torch.cuda.current_stream()                         # (initialises the runtime the first time)
    _RAW[0], _RAW[1] = torch._C._cuda_getCurrentRawStream, torch._C._cuda_getDevice
    return _RAW[0]


def stream_ptr():
    get = _RAW[0] or _raw_fns()
    return get(_RAW[1]())


def current_stream():
    """The current stream of the current device as a (cached) torch Stream object."""
    get = _RAW[0] or _raw_fns()
    dev = _RAW[1]()
    key = (dev, get(dev))                               # (the default stream's handle is 0 on every device)
    s = _STREAM_OBJECTS.get(key)
    if s is None:
        import torch
        s = _STREAM_OBJECTS[key] = torch.cuda.current_stream()
    return s


class on_stream:
    """``with torch.cuda.stream(s):`` for a stream of the CURRENT device, without the context manager's Python layers
    (two C calls each way); another device's stream takes torch's own context."""
    __slots__ = ("s", "prev", "ctx")

    def __init__(self, stream):
        self.s, self.prev, self.ctx = stream, None, None

    def __enter__(self):
        import torch
        s = self.s
        if (_RAW[1] or (_raw_fns() and _RAW[1]))() != s.device_index:
            self.ctx = torch.cuda.stream(s)
            return self.ctx.__enter__()
        self.prev = torch._C._cuda_getCurrentStream(s.device_index)
        torch._C._cuda_setStream(stream_id=s.stream_id, device_index=s.device_index, device_type=s.device_type)
        return None

    def __exit__(self, *exc):
        if self.ctx is not None:
            return self.ctx.__exit__(*exc)
        import torch
        p = self.prev
        torch._C._cuda_setStream(stream_id=p[0], device_index=p[1], device_type=p[2])
        return False
