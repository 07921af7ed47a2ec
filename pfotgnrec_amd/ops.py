"""``torch.library`` registration of the stateless native ops (namespace ``pfotgn``).

BASELINE.json's north_star words the boundary as "PyTorch-ROCm custom ops".  The core is the C ABI (``include/pfotgn.h``,
bound in ``_lib.py``); this module registers the entry points that are pure functions of their tensor arguments as
dispatcher ops, so they show up in ``torch.ops.pfotgn.*``, carry fake (meta) implementations for tracing / shape
inference and - for the BPR loss - an autograd formula:

    torch.ops.pfotgn.tnbr_sample(indptr, nbr, eidx, ts, q_nodes, q_ts, K)      utils/utils.py:163-219 (most recent)
    torch.ops.pfotgn.time_encode(t, weight, bias)                              model/time_encoding.py:17-25
    torch.ops.pfotgn.bpr_loss(emb, batch, n_neg, pos_block, grad_scale)        main.py:321-337 / 364-381
    torch.ops.pfotgn.rank_metrics(emb, batch, n_items)                         evaluation.py:114-145
    torch.ops.pfotgn.list_metrics(list_item, truth, cutoffs, upper_u, ...)     a served list against what happened (no reference form)
    torch.ops.pfotgn.recommend_topk(user_emb, item_emb, k, n_blocks, ...)      the k best candidates per user (no reference form)
    torch.ops.pfotgn.recommend_mv_topk(user_emb, item_emb, k, cand_stock, ...) the same under the rank fusion of main.py:243-289
    torch.ops.pfotgn.recommend_mv_topk_wide(...)                               its form for lists beyond 2048 candidates
    torch.ops.pfotgn.recommend_list_topk(user_emb, item_emb, k, list_pos, ...) the k best of every user's own list
    torch.ops.pfotgn.recommend_list_mv_topk(...)                               the same in the mean-variance order
    torch.ops.pfotgn.history_gather(indptr, adj_nbr, adj_ts, users, ts, width, ...)  what each user interacted with before its time
    torch.ops.pfotgn.holdings_apply(src, stock, side, ts, hold_idx, hold_len, hold_time, ...)  buys and sells applied to ledger rows, in place
    torch.ops.pfotgn.holdings_gather_weights(users, hold_idx, hold_len, hold_qty, mode, ...)   the weight rows of the weighted mean-variance order

Only a HIP implementation is registered ("cuda" dispatch key = ROCm here): on any other device the dispatcher raises,
there is no CPU fallback.  The TGN step itself keeps its ``autograd.Function`` (``tgn._EmbedFn``): it owns state (memory,
message tables, a workspace per outstanding call) that a functional op schema cannot express.
"""
from typing import Optional

import torch

from . import _lib, functional

_LIB_NS = "pfotgn"


@torch.library.custom_op(_LIB_NS + "::tnbr_sample", mutates_args=(), device_types="cuda")
def tnbr_sample(indptr: torch.Tensor, adj_nbr: torch.Tensor, adj_eidx: torch.Tensor, adj_ts: torch.Tensor, q_nodes: torch.Tensor,
                q_ts: torch.Tensor, K: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    N = q_nodes.shape[0]
    q_nodes, q_ts = q_nodes.to(torch.int32).contiguous(), q_ts.to(torch.float64).contiguous()
    o_nbr = torch.empty((N, K), dtype=torch.int32, device=q_nodes.device)
    o_eidx = torch.empty((N, K), dtype=torch.int32, device=q_nodes.device)
    o_et = torch.empty((N, K), dtype=torch.float32, device=q_nodes.device)
    _lib.call("pfo_tnbr_sample", _lib.ptr(indptr), _lib.ptr(adj_nbr), _lib.ptr(adj_eidx), _lib.ptr(adj_ts), indptr.shape[0] - 1,
              _lib.ptr(q_nodes), _lib.ptr(q_ts), N, K, 0, None, 0, 0, _lib.ptr(o_nbr), _lib.ptr(o_eidx), _lib.ptr(o_et), None,
              None, None, _lib.stream_ptr())
    return o_nbr, o_eidx, o_et


@tnbr_sample.register_fake
def _(indptr, adj_nbr, adj_eidx, adj_ts, q_nodes, q_ts, K):
    N = q_nodes.shape[0]
    return (q_nodes.new_empty((N, K), dtype=torch.int32), q_nodes.new_empty((N, K), dtype=torch.int32),
            q_nodes.new_empty((N, K), dtype=torch.float32))


@torch.library.custom_op(_LIB_NS + "::time_encode", mutates_args=(), device_types="cuda")
def time_encode(t: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    return functional.time_encode(t, weight.reshape(-1), bias)


@time_encode.register_fake
def _(t, weight, bias):
    return t.new_empty(t.shape + (bias.shape[0],), dtype=torch.float32)


@torch.library.custom_op(_LIB_NS + "::bpr_loss_fwd", mutates_args=(), device_types="cuda")
def _bpr_loss_fwd(emb: torch.Tensor, batch: int, n_neg: int, pos_block: int, grad_scale: float) -> tuple[torch.Tensor, torch.Tensor]:
    emb = emb.contiguous()
    R, D = emb.shape
    loss = torch.empty(1, dtype=torch.float32, device=emb.device)
    d_emb = torch.empty_like(emb)
    scratch = torch.empty(batch, dtype=torch.float32, device=emb.device)
    _lib.call("pfo_bpr_loss", emb.data_ptr(), batch, D, pos_block * batch, (pos_block + 1) * batch, n_neg, R, float(grad_scale),
              loss.data_ptr(), d_emb.data_ptr(), scratch.data_ptr(), _lib.stream_ptr())
    return loss.reshape(()), d_emb


@_bpr_loss_fwd.register_fake
def _(emb, batch, n_neg, pos_block, grad_scale):
    return emb.new_empty(()), torch.empty_like(emb)


def _bpr_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])


def _bpr_backward(ctx, g_loss, g_demb):
    (d_emb,) = ctx.saved_tensors
    return d_emb * g_loss, None, None, None, None


_bpr_loss_fwd.register_autograd(_bpr_backward, setup_context=_bpr_setup)


def bpr_loss(emb, batch, n_neg, pos_block=1, grad_scale=1.0):
    """Dispatcher form of ``pfotgnrec_amd.bpr_loss`` (same semantics)."""
    return torch.ops.pfotgn.bpr_loss_fwd(emb, batch, n_neg, pos_block, grad_scale)[0]


@torch.library.custom_op(_LIB_NS + "::rank_metrics", mutates_args=(), device_types="cuda")
def rank_metrics(emb: torch.Tensor, batch: int, n_items: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return functional.rank_metrics(emb, batch, n_items)


@rank_metrics.register_fake
def _(emb, batch, n_items):
    return (emb.new_empty((batch,), dtype=torch.int32), emb.new_empty((batch, 3), dtype=torch.float32),
            emb.new_empty((batch, 3), dtype=torch.float32))


@torch.library.custom_op(_LIB_NS + "::list_metrics", mutates_args=(), device_types="cuda")
def list_metrics(list_item: torch.Tensor, truth: torch.Tensor, cutoffs: list[int], upper_u: int, ret_past: torch.Tensor,
                 day_past: torch.Tensor, ret_future: torch.Tensor, day_future: torch.Tensor, port_idx: Optional[torch.Tensor] = None,
                 port_len: Optional[torch.Tensor] = None,
                 n_valid: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return functional.list_metrics(list_item, truth, cutoffs, port_idx, port_len, upper_u, ret_past, day_past, ret_future, day_future,
                                   n_valid)


@list_metrics.register_fake
def _(list_item, truth, cutoffs, upper_u, ret_past, day_past, ret_future, day_future, port_idx=None, port_len=None, n_valid=None):
    U, n_c = list_item.shape[0], len(cutoffs)
    return (list_item.new_empty((U,), dtype=torch.int32), list_item.new_empty((U, n_c), dtype=torch.float32),
            list_item.new_empty((U, n_c), dtype=torch.float32), list_item.new_empty((U, 4 * n_c), dtype=torch.float64))


@torch.library.custom_op(_LIB_NS + "::recommend_topk", mutates_args=(), device_types="cuda")
def recommend_topk(user_emb: torch.Tensor, item_emb: torch.Tensor, k: int, n_blocks: int = 1,
                   user_block: Optional[torch.Tensor] = None, excl_pos: Optional[torch.Tensor] = None,
                   excl_len: Optional[torch.Tensor] = None,
                   item_ok: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return functional.recommend_topk(user_emb, item_emb, k, user_block, excl_pos, excl_len, item_ok, n_blocks=n_blocks)


@recommend_topk.register_fake
def _(user_emb, item_emb, k, n_blocks=1, user_block=None, excl_pos=None, excl_len=None, item_ok=None):
    U = user_emb.shape[0]
    return (user_emb.new_empty((U, k), dtype=torch.int32), user_emb.new_empty((U, k), dtype=torch.float32),
            user_emb.new_empty((U,), dtype=torch.int32))


@torch.library.custom_op(_LIB_NS + "::recommend_mv_topk", mutates_args=(), device_types="cuda")
def recommend_mv_topk(user_emb: torch.Tensor, item_emb: torch.Tensor, k: int, cand_stock: torch.Tensor, returns: torch.Tensor,
                      day_idx: torch.Tensor, gamma: float, lambda_mv: float, n_blocks: int = 1,
                      port_idx: Optional[torch.Tensor] = None, port_len: Optional[torch.Tensor] = None,
                      user_block: Optional[torch.Tensor] = None, excl_pos: Optional[torch.Tensor] = None,
                      excl_len: Optional[torch.Tensor] = None, item_ok: Optional[torch.Tensor] = None,
                      port_w: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return functional.recommend_mv_topk(user_emb, item_emb, k, cand_stock, returns, day_idx, port_idx, port_len, gamma, lambda_mv,
                                        user_block, excl_pos, excl_len, item_ok, n_blocks=n_blocks, port_w=port_w)


@recommend_mv_topk.register_fake
def _(user_emb, item_emb, k, cand_stock, returns, day_idx, gamma, lambda_mv, n_blocks=1, port_idx=None, port_len=None,
      user_block=None, excl_pos=None, excl_len=None, item_ok=None, port_w=None):
    U = user_emb.shape[0]
    return (user_emb.new_empty((U, k), dtype=torch.int32), user_emb.new_empty((U, k), dtype=torch.float32),
            user_emb.new_empty((U, k), dtype=torch.float64), user_emb.new_empty((U,), dtype=torch.int32))


@torch.library.custom_op(_LIB_NS + "::recommend_mv_topk_wide", mutates_args=(), device_types="cuda")
def recommend_mv_topk_wide(user_emb: torch.Tensor, item_emb: torch.Tensor, k: int, cand_stock: torch.Tensor, returns: torch.Tensor,
                           day_idx: torch.Tensor, gamma: float, lambda_mv: float, n_blocks: int = 1,
                           port_idx: Optional[torch.Tensor] = None, port_len: Optional[torch.Tensor] = None,
                           user_block: Optional[torch.Tensor] = None, excl_pos: Optional[torch.Tensor] = None,
                           excl_len: Optional[torch.Tensor] = None, item_ok: Optional[torch.Tensor] = None,
                           port_w: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return functional.recommend_mv_topk_wide(user_emb, item_emb, k, cand_stock, returns, day_idx, port_idx, port_len, gamma, lambda_mv,
                                             user_block, excl_pos, excl_len, item_ok, n_blocks=n_blocks, port_w=port_w)   # (its own workspace)


@recommend_mv_topk_wide.register_fake
def _(user_emb, item_emb, k, cand_stock, returns, day_idx, gamma, lambda_mv, n_blocks=1, port_idx=None, port_len=None,
      user_block=None, excl_pos=None, excl_len=None, item_ok=None, port_w=None):
    U = user_emb.shape[0]
    return (user_emb.new_empty((U, k), dtype=torch.int32), user_emb.new_empty((U, k), dtype=torch.float32),
            user_emb.new_empty((U, k), dtype=torch.float64), user_emb.new_empty((U,), dtype=torch.int32))


@torch.library.custom_op(_LIB_NS + "::recommend_list_topk", mutates_args=(), device_types="cuda")
def recommend_list_topk(user_emb: torch.Tensor, item_emb: torch.Tensor, k: int, list_pos: torch.Tensor,
                        list_len: Optional[torch.Tensor] = None, n_blocks: int = 1, user_block: Optional[torch.Tensor] = None,
                        item_ok: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return functional.recommend_list_topk(user_emb, item_emb, k, list_pos, list_len, user_block, item_ok, n_blocks=n_blocks)


@recommend_list_topk.register_fake
def _(user_emb, item_emb, k, list_pos, list_len=None, n_blocks=1, user_block=None, item_ok=None):
    U = user_emb.shape[0]
    return (user_emb.new_empty((U, k), dtype=torch.int32), user_emb.new_empty((U, k), dtype=torch.float32),
            user_emb.new_empty((U,), dtype=torch.int32))


@torch.library.custom_op(_LIB_NS + "::recommend_list_mv_topk", mutates_args=(), device_types="cuda")
def recommend_list_mv_topk(user_emb: torch.Tensor, item_emb: torch.Tensor, k: int, list_pos: torch.Tensor, cand_stock: torch.Tensor,
                           returns: torch.Tensor, day_idx: torch.Tensor, gamma: float, lambda_mv: float,
                           list_len: Optional[torch.Tensor] = None, n_blocks: int = 1, port_idx: Optional[torch.Tensor] = None,
                           port_len: Optional[torch.Tensor] = None, user_block: Optional[torch.Tensor] = None,
                           item_ok: Optional[torch.Tensor] = None,
                           port_w: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return functional.recommend_list_mv_topk(user_emb, item_emb, k, list_pos, list_len, cand_stock, returns, day_idx, port_idx, port_len,
                                             gamma, lambda_mv, user_block, item_ok, n_blocks=n_blocks, port_w=port_w)


@recommend_list_mv_topk.register_fake
def _(user_emb, item_emb, k, list_pos, cand_stock, returns, day_idx, gamma, lambda_mv, list_len=None, n_blocks=1, port_idx=None,
      port_len=None, user_block=None, item_ok=None, port_w=None):
    U = user_emb.shape[0]
    return (user_emb.new_empty((U, k), dtype=torch.int32), user_emb.new_empty((U, k), dtype=torch.float32),
            user_emb.new_empty((U, k), dtype=torch.float64), user_emb.new_empty((U,), dtype=torch.int32))


@torch.library.custom_op(_LIB_NS + "::history_gather", mutates_args=(), device_types="cuda")
def history_gather(indptr: torch.Tensor, adj_nbr: torch.Tensor, adj_ts: torch.Tensor, users: torch.Tensor, ts: torch.Tensor,
                   width: int, since: Optional[torch.Tensor] = None, max_scan: int = 0, items: Optional[torch.Tensor] = None,
                   upper_u: Optional[int] = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor,
                                                           torch.Tensor]:
    """(node, len, time, count, pos, stock) of ``functional.history_gather``; pos / stock have no column without ``items`` /
    ``upper_u`` (an op returns tensors, not None)."""
    want = ("node", "len", "time", "count") + (("pos",) if items is not None else ()) + (("stock",) if upper_u is not None else ())
    got = dict(zip(want, functional.history_gather(indptr, adj_nbr, adj_ts, users, ts, width, since, max_scan, items, None, upper_u, want)))
    none = lambda: got["node"].new_empty((users.shape[0], 0))
    return got["node"], got["len"], got["time"], got["count"], got.get("pos", none()), got.get("stock", none())


@history_gather.register_fake
def _(indptr, adj_nbr, adj_ts, users, ts, width, since=None, max_scan=0, items=None, upper_u=None):
    U = users.shape[0]
    rows = lambda dt, w=width: users.new_empty((U, w), dtype=dt)
    return (rows(torch.int32), users.new_empty((U,), dtype=torch.int32), rows(torch.float64), rows(torch.int32),
            rows(torch.int32, width if items is not None else 0), rows(torch.int32, width if upper_u is not None else 0))


@torch.library.custom_op(_LIB_NS + "::holdings_apply", mutates_args=("hold_idx", "hold_len", "hold_time", "hold_qty", "counters"),
                         device_types="cuda")
def holdings_apply(src: torch.Tensor, stock: torch.Tensor, side: torch.Tensor, ts: torch.Tensor, hold_idx: torch.Tensor,
                   hold_len: torch.Tensor, hold_time: torch.Tensor, hold_qty: Optional[torch.Tensor], counters: Optional[torch.Tensor],
                   qty: Optional[torch.Tensor] = None) -> None:
    """``functional.holdings_apply``: the ledger tables (and the counters) are written in place, nothing is returned.  The two
    optional tables that are written take no default (pass None): the dispatcher bumps the version of every mutated
    argument by position."""
    functional.holdings_apply(src, stock, side, ts, hold_idx, hold_len, hold_time, qty, hold_qty, counters)


@holdings_apply.register_fake
def _(src, stock, side, ts, hold_idx, hold_len, hold_time, hold_qty, counters, qty=None):
    return None


@torch.library.custom_op(_LIB_NS + "::holdings_gather_weights", mutates_args=(), device_types="cuda")
def holdings_gather_weights(users: torch.Tensor, hold_idx: torch.Tensor, hold_len: torch.Tensor, hold_qty: torch.Tensor, mode: int,
                            last_close: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``functional.holdings_gather_weights``: mode 0 = shares, 1 = value (needs ``last_close``)."""
    return functional.holdings_gather_weights(users, hold_idx, hold_len, hold_qty, mode, last_close)


@holdings_gather_weights.register_fake
def _(users, hold_idx, hold_len, hold_qty, mode, last_close=None):
    return users.new_empty((users.shape[0], hold_idx.shape[1]), dtype=torch.float64)
