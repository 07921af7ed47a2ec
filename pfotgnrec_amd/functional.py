"""Autograd-facing wrappers of the small native ops (BPR loss, TimeEncode)."""
import torch

from . import _lib


_TICKETS = {}      # device -> i32[1]: the loss kernel's "last workgroup takes the mean" counter (zero at rest)


def bpr_loss_and_grad(emb, B, pos_off, neg_off, n_neg, scale):
    """One launch (``pfo_bpr_loss_fused``): (loss f32[1], d loss / d emb * scale f32[R,D])."""
    _lib.require_gpu(emb.device)
    emb = emb.contiguous()
    R, D = emb.shape
    ticket = _TICKETS.get(emb.device)
    if ticket is None:
        ticket = _TICKETS[emb.device] = torch.zeros(1, dtype=torch.int32, device=emb.device)
    loss = torch.empty(1, dtype=torch.float32, device=emb.device)
    d_emb = torch.empty_like(emb)
    scratch = torch.empty(B, dtype=torch.float32, device=emb.device)
    _lib.call("pfo_bpr_loss_fused", emb.data_ptr(), B, D, pos_off, neg_off, n_neg, R, float(scale), loss.data_ptr(),
              d_emb.data_ptr(), scratch.data_ptr(), ticket.data_ptr(), _lib.stream_ptr())
    return loss, d_emb


class _BprFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb, B, pos_off, neg_off, n_neg, scale):
        loss, d_emb = bpr_loss_and_grad(emb, B, pos_off, neg_off, n_neg, scale)
        ctx.save_for_backward(d_emb)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (d_emb,) = ctx.saved_tensors
        return d_emb * g, None, None, None, None, None


def bpr_loss(emb, batch, n_neg, pos_block=1, grad_scale=1.0):
    """BPR loss of main.py:321-337 / 364-381 on the root-ordered embedding matrix of ``TGN.embed_device``.

    emb [R,D] = [src B | dst B | (p_pos B) | neg B*n_neg]; ``pos_block`` = 1 when the positive is the destination
    (baseline path), 2 when it is the p_pos block (``ours`` path).  ``grad_scale`` multiplies the gradient only
    (``tgn.dp_grad_scale`` = local/global batch under data parallelism, so that the summed gradients equal the
    global-batch mean gradient also when the shards are uneven).
    """
    if batch == 0:
        # an empty data-parallel shard (global batch shorter than the world size): zero loss, zero gradient, but still
        # a differentiable scalar so that every rank runs the same backward / all-reduce sequence
        return emb.sum() * 0.0
    pos_off = pos_block * batch
    neg_off = (pos_block + 1) * batch
    return _BprFn.apply(emb, batch, pos_off, neg_off, n_neg, grad_scale)


def adjacent_rows(blocks):
    """Row blocks that lie one behind the other in ONE buffer (the outputs of ``compute_temporal_embeddings``, the gradient
    blocks ``bpr_loss_blocks`` hands back) as the single matrix they are a cut of - no copy; None when they are anything else."""
    t0 = blocks[0]
    if t0.dim() != 2:
        return None
    D, off, base = t0.shape[1], t0.storage_offset(), t0.untyped_storage().data_ptr()
    rows = 0
    for t in blocks:
        if (t.dim() != 2 or t.shape[1] != D or t.dtype != t0.dtype or not t.is_contiguous()
                or t.untyped_storage().data_ptr() != base or t.storage_offset() != off + rows * D):
            return None
        rows += t.shape[0]
    return torch.as_strided(t0, (rows, D), (D, 1), off)


class _BprBlocksFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, n_neg, *blocks):
        emb = adjacent_rows(blocks)
        if emb is None:
            emb = torch.cat(blocks)
        B = blocks[0].shape[0]
        loss, d_emb = bpr_loss_and_grad(emb, B, (len(blocks) - 2) * B, (len(blocks) - 1) * B, n_neg, 1.0)
        ctx.save_for_backward(d_emb)
        ctx.heights = [t.shape[0] for t in blocks]
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (d_emb,) = ctx.saved_tensors
        d = d_emb * g
        out, r = [], 0
        for h in ctx.heights:
            out.append(d[r:r + h])
            r += h
        return (None,) + tuple(out)


def bpr_loss_blocks(source_embedding, destination_embedding, negative_embedding, p_pos_embedding=None):
    """The BPR expression of main.py:364-381 (baseline: positive = destination) / 321-337 (``ours``: positive = the p_pos block,
    pass it as ``p_pos_embedding``) on the blocks the reference's loop holds after ``compute_temporal_embeddings[_p]`` - one
    native launch for loss and gradient rows instead of ten torch kernels forward and ~20 backward:

        loss = pfotgnrec_amd.bpr_loss_blocks(source_embedding, destination_embedding, negative_embedding)

    The blocks are used in place when they are the adjacent outputs of one call (no copy either way: the gradient blocks
    go back as adjacent rows of one matrix and the TGN backward takes that matrix as it stands)."""
    B = source_embedding.shape[0]
    if B == 0:
        return source_embedding.sum() * 0.0
    D = source_embedding.shape[-1]
    blocks = [source_embedding.reshape(B, D), destination_embedding.reshape(B, D)]
    if p_pos_embedding is not None:
        blocks.append(p_pos_embedding.reshape(B, D))
    neg = negative_embedding.reshape(-1, D)
    blocks.append(neg)
    return _BprBlocksFn.apply(neg.shape[0] // B, *blocks)


def bpr_step(tgn, emb, batch, n_neg, pos_block=1, grad_scale=None, optimizer=None, collective=None):
    """``loss = bpr_loss(...); loss.backward()`` (main.py:321-337 + 388) as two native calls and no torch kernel: the loss
    kernel writes the already scaled gradient rows and the TGN backward is called on them directly, skipping autograd's
    seed fill and ``d_emb * g`` multiply (three ~6 us launches on the critical path of a 1.5 ms step); the batch mean of the
    per-interaction losses - an input of nothing - is taken beside the backward.  ``emb`` must be the
    tensor ``TGN.embed_device`` returned under autograd; anything else (an empty shard, a view) takes the autograd route.

    ``optimizer`` (a ``FusedAdam`` of this model, single rank): ``loss.backward(); optimizer.step()`` (main.py:388-389) in
    one go, with the END of the backward and the optimizer's kernel left on the library's side stream
    (``pfo_tgn_batch.defer_join`` + ``pfo_tgn_adam_side``): the caller's stream does not wait out the last ~40 us of
    side-stream launches (the chain back to the layer-1 projection weights) nor the Adam kernel - it goes straight on to the
    next batch's candidate draw and neighbour sampling, and the next forward joins where it first needs parameters.
    Gradients and parameters are IN FLIGHT on that stream afterwards: read them only after ``tgn.join()`` (``state_dict()``
    joins by itself).  ``optimizer.zero_grad(set_to_none=True)`` afterwards is fine (host side only).
    ``collective`` (a data-parallel rank, with ``optimizer``): a callable that all-reduces ``tgn.flat_grad`` in place
    (``lambda: allreduce_flat_grad(tgn.flat_grad, world)``).  It is issued on the library's side stream between the end of
    the backward and the optimizer's kernel there: the gradient exchange of step n then runs beside step n+1's candidate
    draw and neighbour sampling instead of holding the caller's stream.  Every rank issues it exactly once per call - also a
    rank whose shard is empty (no native backward: the serial order on the caller's stream, same collective).
    Returns the detached loss."""
    call = getattr(emb.grad_fn, "call", None) if emb.grad_fn is not None else None
    if batch == 0 or call is None or call.ws is None or emb.shape[0] != call.R:
        loss = bpr_loss(emb, batch, n_neg, pos_block, tgn.dp_grad_scale if grad_scale is None else grad_scale)
        loss.backward()
        if optimizer is not None and getattr(optimizer, "tgn", None) is tgn:
            if collective is not None:
                collective()
            optimizer.step()
        return loss.detach()
    scale = tgn.dp_grad_scale if grad_scale is None else grad_scale
    e = emb.detach().contiguous()
    R, D = e.shape
    parts = torch.empty(batch, dtype=torch.float32, device=e.device)
    d_emb = torch.empty_like(e)
    loss = torch.empty(1, dtype=torch.float32, device=e.device)
    _lib.call("pfo_bpr_loss_parts", e.data_ptr(), batch, D, pos_block * batch, (pos_block + 1) * batch, n_neg, R, float(scale),
              parts.data_ptr(), d_emb.data_ptr(), _lib.stream_ptr())
    ours = optimizer is not None and getattr(optimizer, "tgn", None) is tgn
    fused_opt = (ours and (tgn.dp_world == 1 or collective is not None)
                 and not torch.cuda.is_current_stream_capturing() and not _lib.prof_is_on())
    tgn._native_backward(call, d_emb, mean=(parts, loss), defer_join=fused_opt)     # the batch mean of the losses: on the backward's side stream
    call.release()
    if collective is not None and ours:
        if fused_opt:
            with torch.cuda.stream(tgn.side_stream()):      # behind the backward's last side-stream launch, in front of Adam there
                collective()
        else:
            collective()
    if optimizer is not None:
        optimizer.step(side=fused_opt)
    return loss[0]


def time_encode(t, weight, bias):
    """cos(fma(t, w, b)) (model/time_encoding.py:17-25), forward only; t f32[...], returns [..., D]."""
    _lib.require_gpu(t.device)
    t = t.contiguous().float()
    D = bias.shape[0]
    out = torch.empty(t.shape + (D,), dtype=torch.float32, device=t.device)
    _lib.call("pfo_time_encode", t.data_ptr(), t.numel(), weight.contiguous().data_ptr(), bias.contiguous().data_ptr(),
              D, out.data_ptr(), _lib.stream_ptr())
    return out


def rank_metrics(emb, batch, n_items):
    """Ranking part of evaluation.py:114-145 on the device: emb [R,D] = [src B | dst B | neg B*n_items].

    Returns (rank i32[B], recall f32[B,3], ndcg f32[B,3]) for k = 1, 3, 5; rank = number of negatives scoring >= the
    positive (canonical tie policy)."""
    _lib.require_gpu(emb.device)
    emb = emb.contiguous()
    D = emb.shape[1]
    rank = torch.empty(batch, dtype=torch.int32, device=emb.device)
    hits = torch.empty((batch, 3), dtype=torch.float32, device=emb.device)
    ndcg = torch.empty((batch, 3), dtype=torch.float32, device=emb.device)
    _lib.call("pfo_rank_metrics", emb.data_ptr(), batch, D, n_items, rank.data_ptr(), hits.data_ptr(), ndcg.data_ptr(),
              _lib.stream_ptr())
    return rank, hits, ndcg


def eval_buffers(rows, device):
    """Preallocated outputs of ``eval_metrics`` for ``rows`` interactions: (rank i32[rows], recall f32[rows,3],
    ndcg f32[rows,3], top5_pos i32[rows,5], top5_item i32[rows,5], invest f64[rows,12])."""
    _lib.require_gpu(device)
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)
    return (e(rows, torch.int32), e((rows, 3), torch.float32), e((rows, 3), torch.float32), e((rows, 5), torch.int32),
            e((rows, 5), torch.int32), e((rows, 12), torch.float64))


def eval_metrics(emb, batch, n_neg, cand, day_idx, port_idx, port_len, ret_past, ret_future, upper_u, out=None, out_row0=0):
    """The per-interaction part of evaluation.py:114-207 in one launch (``pfo_eval_metrics``): emb [R,D] = [src B | dst B |
    neg B*n_neg]; cand i32[B,1+n_neg] item node ids, column 0 the destination; day_idx i32[B]; port_idx i32[B,W] stock
    indices and port_len i32[B] (0 for the reference's ``'' in portfolio`` rows); ret_past / ret_future f64[n_days, n_stocks,
    n_ret] log-return tables (``InvestTables``); all on the device.

    Returns (rank i32[B], recall f32[B,3], ndcg f32[B,3], top5_pos i32[B,5], top5_item i32[B,5], invest f64[B,12]): rank,
    recall and NDCG as ``rank_metrics``; the five best candidates in the canonical order (score descending, the larger
    position first among equal scores) as positions into the 1+n_neg row and as node ids; invest =
    (return@1,3,5 | sharpe@1,3,5) in-sample, then out-of-sample (``return_sharpe_at_k``, evaluation.py:23-36).
    ``out`` (``eval_buffers``) and ``out_row0``: write rows [out_row0, out_row0 + B) of preallocated buffers - an evaluation
    pass accumulates on the device and is read back once; the returned tensors are those rows."""
    _lib.require_gpu(emb.device)
    emb = emb.contiguous()
    D = emb.shape[1]
    if out is None:
        out, out_row0 = eval_buffers(batch, emb.device), 0
    W = port_idx.shape[1] if port_idx is not None and port_idx.dim() == 2 else 0
    n_days, n_stocks, n_ret = ret_past.shape
    if tuple(ret_future.shape) != (n_days, n_stocks, n_ret):
        raise ValueError("ret_past and ret_future differ in shape")
    if emb.shape[0] != batch * (2 + n_neg) or tuple(cand.shape) != (batch, 1 + n_neg):
        raise ValueError("emb must hold batch * (2 + n_neg) rows and cand batch x (1 + n_neg) ids")
    _lib.call("pfo_eval_metrics", emb.data_ptr(), batch, D, n_neg, _lib.ptr(cand.contiguous()), _lib.ptr(day_idx.contiguous()),
              _lib.ptr(port_idx.contiguous() if W else None), _lib.ptr(port_len.contiguous()), W, _lib.ptr(ret_past), _lib.ptr(ret_future),
              n_days, n_stocks, n_ret, int(upper_u), int(out_row0), out[0].shape[0], *[o.data_ptr() for o in out], _lib.stream_ptr())
    return tuple(o[out_row0:out_row0 + batch] for o in out)


def eval_buffers_mv(rows, device):
    """Preallocated outputs of ``eval_metrics_mv`` for ``rows`` interactions: the six of ``eval_buffers`` followed by
    (top5_fused f64[rows,5], n_adm i32[rows])."""
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)
    return eval_buffers(rows, device) + (e((rows, 5), torch.float64), e(rows, torch.int32))


def eval_metrics_mv(emb, batch, n_neg, cand, day_idx, port_idx, port_len, ret_past, ret_future, upper_u, returns_mv, mv_day_idx, gamma,
                    lambda_mv, mode, out=None, out_row0=0, want_all=False):
    """``eval_metrics`` with the row ranked in a served order, in one launch (``pfo_eval_metrics_mv``): ``mode`` 0 the
    mean-variance rank fusion ``recommend_mv_topk`` serves, 1 the basket rounds of ``recommend_basket_topk`` with k = 5.

    The first ten arguments are ``eval_metrics``'s and the score is that kernel's to the bit.  returns_mv f64[mv_days, mv_stocks,
    mv_ret] (``MVSampler.returns``): the table the ORDER is computed from, with its own day numbering mv_day_idx i32[B]; the
    portfolio rows and the candidates' stocks (node id - upper_u - 1) are the ones the investment stage uses.  Over the admissible
    candidates (stock inside the table, y no NaN; none for a day outside it): fused = lambda_mv * rank(y_mv) + (1 - lambda_mv) *
    rank(score), average-tie ranks; fused descending, the larger position first among equal values.

    Returns the six rows of ``eval_metrics`` - with top5 and invest of THIS order, and rank = the positive's place in it, or
    ``_lib.EVAL_RANK_NONE`` when it is not admissible or (mode 1) not among the five picks: recall and NDCG are 0 then - followed by
    (top5_fused f64[B,5], n_adm i32[B]); empty slots -1 / -1 / -inf.  ``out``: ``eval_buffers_mv``.  ``want_all`` adds (score
    f32[B,1+n_neg], y f64[B,1+n_neg], fused f64[B,1+n_neg]), NaN in the last two where a candidate is not admissible (mode 1:
    round 0's)."""
    import operator
    if not isinstance(emb, torch.Tensor) or emb.dim() != 2:
        raise ValueError("emb must be a 2-D tensor")
    try:
        batch, n_neg, mode = operator.index(batch), operator.index(n_neg), operator.index(mode)
    except TypeError:
        raise ValueError("batch, n_neg and mode must be integers") from None
    if mode not in (0, 1):
        raise ValueError("mode must be 0 (the fused list) or 1 (the basket), got %d" % mode)
    if n_neg < 1 or 1 + n_neg > _lib.RECOMMEND_MV_MAX_ITEMS:
        raise ValueError("1 + n_neg must be in [2, %d] under a mean-variance order (got %d)" % (_lib.RECOMMEND_MV_MAX_ITEMS, 1 + n_neg))
    if not isinstance(returns_mv, torch.Tensor) or returns_mv.dim() != 3 or returns_mv.dtype != torch.float64 or 0 in returns_mv.shape:
        raise ValueError("returns_mv must be a float64 tensor [mv_days, mv_stocks, mv_ret]")
    if not 2 <= returns_mv.shape[2] <= 128:
        raise ValueError("mv_ret must be in [2, 128] (got %d)" % returns_mv.shape[2])
    if not isinstance(mv_day_idx, torch.Tensor) or tuple(mv_day_idx.shape) != (batch,) or mv_day_idx.dtype != torch.int32:
        raise ValueError("mv_day_idx must be int32 [B]")
    n_days, n_stocks, n_ret = ret_past.shape
    if tuple(ret_future.shape) != (n_days, n_stocks, n_ret):
        raise ValueError("ret_past and ret_future differ in shape")
    if emb.shape[0] != batch * (2 + n_neg) or tuple(cand.shape) != (batch, 1 + n_neg):
        raise ValueError("emb must hold batch * (2 + n_neg) rows and cand batch x (1 + n_neg) ids")
    _lib.require_gpu(emb.device)
    for t in (returns_mv, mv_day_idx):
        if t.device != emb.device:
            raise ValueError("all tensors must live on %s" % emb.device)
    emb = emb.contiguous()
    D = emb.shape[1]
    if out is None:
        out, out_row0 = eval_buffers_mv(batch, emb.device), 0
    W = port_idx.shape[1] if port_idx is not None and port_idx.dim() == 2 else 0
    extra = tuple(torch.empty((batch, 1 + n_neg), dtype=dt, device=emb.device) if want_all else None
                  for dt in (torch.float32, torch.float64, torch.float64))
    mv_days, mv_stocks, mv_ret = (int(v) for v in returns_mv.shape)
    _lib.call("pfo_eval_metrics_mv", emb.data_ptr(), batch, D, n_neg, _lib.ptr(cand.contiguous()), _lib.ptr(day_idx.contiguous()),
              _lib.ptr(port_idx.contiguous() if W else None), _lib.ptr(port_len.contiguous()), W, _lib.ptr(ret_past), _lib.ptr(ret_future),
              n_days, n_stocks, n_ret, int(upper_u), int(out_row0), out[0].shape[0], *[o.data_ptr() for o in out[:6]],
              returns_mv.contiguous().data_ptr(), mv_days, mv_stocks, mv_ret, _lib.ptr(mv_day_idx.contiguous()), float(gamma),
              float(lambda_mv), mode, out[6].data_ptr(), out[7].data_ptr(), *(_lib.ptr(t) for t in extra), _lib.stream_ptr())
    rows = tuple(o[out_row0:out_row0 + batch] for o in out)
    return rows + extra if want_all else rows


def check_cutoffs(cutoffs, depth, what="L"):
    """``cutoffs`` as a tuple of ints: 1 to 8 of them, strictly increasing, each in [1, depth] (ValueError)."""
    import operator
    try:
        cuts = tuple(operator.index(c) for c in cutoffs)
    except TypeError:
        raise ValueError("cutoffs must be a sequence of integers") from None
    if not 1 <= len(cuts) <= 8:
        raise ValueError("between 1 and 8 cutoffs, got %d" % len(cuts))
    if any(b <= a for a, b in zip(cuts, cuts[1:])):
        raise ValueError("cutoffs must be strictly increasing, got %s" % (cuts,))
    if cuts[0] < 1 or cuts[-1] > depth:
        raise ValueError("cutoffs must lie in [1, %s] = [1, %d], got %s" % (what, depth, cuts))
    return cuts


def list_buffers(rows, n_cutoffs, device):
    """Preallocated outputs of ``list_metrics`` for ``rows`` lists and ``n_cutoffs`` cutoffs: (rank i32[rows], recall
    f32[rows, n_c], ndcg f32[rows, n_c], invest f64[rows, 4 n_c])."""
    _lib.require_gpu(device)
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)
    return (e(rows, torch.int32), e((rows, n_cutoffs), torch.float32), e((rows, n_cutoffs), torch.float32),
            e((rows, 4 * n_cutoffs), torch.float64))


def list_metrics(list_item, truth, cutoffs, port_idx, port_len, upper_u, ret_past, day_past, ret_future, day_future, n_valid=None,
                 out=None, out_row0=0):
    """A served list scored against what happened, in one launch (``pfo_list_metrics``); whatever order produced the list.

    list_item i32[U, L]: item node ids, best first, as ``TGN.recommend`` returns them (L <= 64); n_valid i32[U] or None (all L):
    the slots in front of it count; a slot holding -1 is skipped and keeps its place.  truth i32[U]: the item the user took,
    < 0 for none.  cutoffs: up to 8 ints, strictly increasing, each in [1, L]; cutoff c = the first c slots.  port_idx i32[U, W]
    stock indices and port_len i32[U] as ``eval_metrics`` reads them (None, None: empty portfolios); a list item's stock is its
    id - upper_u - 1; duplicates count as often as they occur.  ret_past f64[pd, ps, n_ret] read at day_past i32[U], ret_future
    f64[fd, fs, n_ret] at day_future i32[U] - two tables with their own extents and day numbering, or one storage twice (a
    ``PriceLedger``'s ``returns`` with ring slots).  A day or stock outside a table makes that table's figures of the row NaN
    and leaves the other table's alone.

    Returns (rank i32[U], recall f32[U, n_c], ndcg f32[U, n_c], invest f64[U, 4 n_c]): rank = the first counted slot holding
    truth or ``_lib.EVAL_RANK_NONE``; recall = rank < c, NDCG = 1 / log2(rank + 2) where hit; invest = (return@c.. |
    sharpe@c..) in-sample, then out-of-sample - ``eval_metrics``'s investment stage at the cutoffs, bit for bit its [., 12] at
    (1, 3, 5) on its own top-5.  ``out`` (``list_buffers``) and ``out_row0``: write rows [out_row0, out_row0 + U) of
    preallocated buffers; the returned tensors are those rows.  ValueError for anything the shapes rule out, before any launch."""
    import ctypes
    import operator
    if not isinstance(list_item, torch.Tensor) or list_item.dim() != 2 or list_item.dtype != torch.int32:
        raise ValueError("list_item must be an int32 tensor [U, L]")
    U, L = (int(v) for v in list_item.shape)
    if not 1 <= L <= 64:
        raise ValueError("L must be in [1, 64] (got %d)" % L)
    cuts = check_cutoffs(cutoffs, L)
    n_c = len(cuts)
    for name, t in (("truth", truth), ("day_past", day_past), ("day_future", day_future), ("n_valid", n_valid)):
        if name == "n_valid" and t is None:
            continue
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (U,) or t.dtype != torch.int32:
            raise ValueError("%s must be int32 [U] with U = %d" % (name, U))
    W = 0
    if port_idx is not None:
        if not isinstance(port_idx, torch.Tensor) or port_idx.dim() != 2 or port_idx.shape[0] != U or port_idx.dtype != torch.int32:
            raise ValueError("port_idx must be int32 [U, W]")
        W = int(port_idx.shape[1])
        if W and (not isinstance(port_len, torch.Tensor) or tuple(port_len.shape) != (U,) or port_len.dtype != torch.int32):
            raise ValueError("port_len must be int32 [U]")
    for name, t in (("ret_past", ret_past), ("ret_future", ret_future)):
        if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.dtype != torch.float64 or 0 in t.shape or not t.is_contiguous():
            raise ValueError("%s must be a contiguous float64 tensor [days, stocks, n_ret]" % name)
        if max(t.shape[0], t.shape[1]) >= 1 << 31:
            raise ValueError("%s does not fit 32-bit extents" % name)
    n_ret = int(ret_past.shape[2])
    if int(ret_future.shape[2]) != n_ret:
        raise ValueError("ret_past holds %d returns per stock, ret_future %d" % (n_ret, int(ret_future.shape[2])))
    if not 2 <= n_ret <= 128:
        raise ValueError("n_ret must be in [2, 128] (got %d)" % n_ret)
    try:
        upper_u, out_row0 = operator.index(upper_u), operator.index(out_row0)
    except TypeError:
        raise ValueError("upper_u and out_row0 must be integers") from None
    if not -(1 << 31) <= upper_u < (1 << 31):
        raise ValueError("upper_u does not fit 32 bits")
    dev = list_item.device
    if out is not None:
        want = ((), (n_c,), (n_c,), (4 * n_c,))
        dts = (torch.int32, torch.float32, torch.float32, torch.float64)
        if len(out) != 4 or any(not isinstance(o, torch.Tensor) or o.dim() < 1 or o.dtype != dt or tuple(o.shape[1:]) != w
                                or o.shape[0] != out[0].shape[0] or not o.is_contiguous() or o.device != dev
                                for o, w, dt in zip(out, want, dts)):
            raise ValueError("out must be the four contiguous tensors of list_buffers(rows, %d, device)" % n_c)
        if out_row0 < 0 or out_row0 + U > out[0].shape[0]:
            raise ValueError("rows [%d, %d) exceed the output buffers (%d rows)" % (out_row0, out_row0 + U, out[0].shape[0]))
    elif out_row0 != 0:
        raise ValueError("out_row0 without out")
    _lib.require_gpu(dev)
    for t in (truth, day_past, day_future, n_valid, port_idx if W else None, port_len if W else None, ret_past, ret_future):
        if t is not None and t.device != dev:
            raise ValueError("all tensors must live on %s" % dev)
    if out is None:
        out = list_buffers(U, n_c, dev)
    c = lambda t: None if t is None else t.contiguous()
    ins = [c(list_item), c(n_valid), c(truth), c(port_idx) if W else None, c(port_len) if W else None, c(day_past), c(day_future)]
    _lib.call("pfo_list_metrics", _lib.ptr(ins[0]), _lib.ptr(ins[1]), _lib.ptr(ins[2]), U, L, (ctypes.c_int32 * n_c)(*cuts), n_c,
              _lib.ptr(ins[3]), _lib.ptr(ins[4]), W, upper_u, ret_past.data_ptr(), _lib.ptr(ins[5]), int(ret_past.shape[0]),
              int(ret_past.shape[1]), ret_future.data_ptr(), _lib.ptr(ins[6]), int(ret_future.shape[0]), int(ret_future.shape[1]),
              n_ret, out_row0, int(out[0].shape[0]), *[o.data_ptr() for o in out], _lib.stream_ptr())
    return tuple(o[out_row0:out_row0 + U] for o in out)


def _recommend_check(user_emb, item_emb, k, user_block, excl_pos, excl_len, item_ok, dims, also=()):
    """The argument checks the three top-k forms share.  ``dims(U, rows)`` is the caller's part: it checks what only that form
    takes and returns ``(I, n_t)``; ``also``: its tensors, for the device check.  Returns the tensors as the library takes them
    (contiguous; the exclusion pair None without columns, its lengths defaulted; item_ok as u8) and ``U, D, k, I, n_t, W``."""
    import operator
    for name, t in (("user_emb", user_emb), ("item_emb", item_emb)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float32:
            raise ValueError("%s must be a 2-D float32 tensor" % name)
    U, D = user_emb.shape
    if item_emb.shape[1] != D:
        raise ValueError("user_emb has %d columns, item_emb %d" % (D, item_emb.shape[1]))
    if D == 0 or D % 4 != 0 or D > 256:
        raise ValueError("D must be a positive multiple of 4, at most 256 (got %d)" % D)
    try:
        k = operator.index(k)
    except TypeError:
        raise ValueError("k must be an integer") from None
    if not 1 <= k <= 64:
        raise ValueError("k must be in [1, 64] (got %d)" % k)
    I, n_t = dims(U, item_emb.shape[0])
    if user_block is not None and (user_block.dim() != 1 or user_block.shape[0] != U or user_block.dtype != torch.int32):
        raise ValueError("user_block must be int32 [U]")
    if item_ok is not None:
        if item_ok.dim() != 1 or item_ok.shape[0] != I or item_ok.dtype not in (torch.uint8, torch.bool):
            raise ValueError("item_ok must be uint8 or bool [I]")
    W = 0
    if excl_pos is not None:
        if excl_pos.dim() != 2 or excl_pos.shape[0] != U or excl_pos.dtype != torch.int32:
            raise ValueError("excl_pos must be int32 [U, W]")
        W = int(excl_pos.shape[1])
        if excl_len is not None and (excl_len.dim() != 1 or excl_len.shape[0] != U or excl_len.dtype != torch.int32):
            raise ValueError("excl_len must be int32 [U]")
    elif excl_len is not None:
        raise ValueError("excl_len without excl_pos")
    dev = user_emb.device
    _lib.require_gpu(dev)
    for t in (item_emb, user_block, excl_pos, excl_len, item_ok) + tuple(also):
        if t is not None and t.device != dev:
            raise ValueError("all tensors must live on %s" % dev)
    if W and excl_len is None:
        excl_len = torch.full((U,), W, dtype=torch.int32, device=dev)
    if item_ok is not None:
        item_ok = item_ok.contiguous().view(torch.uint8) if item_ok.dtype == torch.bool else item_ok.contiguous()
    return (user_emb.contiguous(), item_emb.contiguous(), user_block.contiguous() if user_block is not None else None,
            excl_pos.contiguous() if W else None, excl_len.contiguous() if W else None, item_ok, U, D, k, I, n_t, W)


def _score_dims(n_blocks, item_ok, user_block):
    """``dims`` of ``_recommend_check`` for the score forms: (I, n_t) from the rows of item_emb and ``n_blocks`` - when None, 1
    without ``user_block`` and rows / len(item_ok) with ``item_ok``."""
    def dims(U, rows):
        n_t = n_blocks
        if n_t is None:
            if item_ok is not None and item_ok.dim() == 1 and item_ok.shape[0] > 0 and rows % item_ok.shape[0] == 0:
                n_t = rows // item_ok.shape[0]
            elif user_block is None:
                n_t = 1
            else:
                raise ValueError("user_block without item_ok needs n_blocks")
        n_t = int(n_t)
        if n_t < 1 or rows % n_t != 0 or rows == 0:
            raise ValueError("item_emb holds %d rows: not n_blocks = %d blocks of at least one candidate" % (rows, n_t))
        if rows // n_t > _lib.RECOMMEND_MAX_ITEMS:
            raise ValueError("%d candidates, at most %d" % (rows // n_t, _lib.RECOMMEND_MAX_ITEMS))
        return rows // n_t, n_t
    return dims


def _recommend_cap(cand_group, group_cap, held_group=None, held_len=None):
    """The cap keywords of the shared-list top-k forms, checked: None without them, else (cand_group, group_cap) - the
    length of ``cand_group`` is checked where I is known (``_capped_dims``), its device with the other tensors'.  With
    ``held_group`` i32[U, W] (W at most ``RECOMMEND_HELD_MAX_WIDTH``; ``held_len`` i32[U], None: the whole row) the tuple is
    (cand_group, group_cap, held_group, held_len) and the ``_held`` entry is called; the rows need the cap pair."""
    import operator
    if held_group is None and held_len is not None:
        raise ValueError("held_len without held_group")
    if held_group is not None and (cand_group is None or group_cap is None):
        raise ValueError("held_group needs cand_group and group_cap: holdings count against a cap")
    if cand_group is None and group_cap is None:
        return None
    if cand_group is None or group_cap is None:
        raise ValueError("cand_group and group_cap go together: give both or neither")
    if not isinstance(cand_group, torch.Tensor) or cand_group.dim() != 1 or cand_group.dtype != torch.int32:
        raise ValueError("cand_group must be int32 [I]")
    try:
        group_cap = operator.index(group_cap)
    except TypeError:
        raise ValueError("group_cap must be an integer") from None
    if group_cap < 1:
        raise ValueError("group_cap must be at least 1 (got %d)" % group_cap)
    if held_group is None:
        return cand_group, min(group_cap, 64)                        # (k <= 64: a cap beyond it never binds)
    if not isinstance(held_group, torch.Tensor) or held_group.dim() != 2 or held_group.dtype != torch.int32:
        raise ValueError("held_group must be int32 [U, W]")
    if held_group.shape[1] > _lib.RECOMMEND_HELD_MAX_WIDTH:
        raise ValueError("held_group must have at most %d columns (got %d)" % (_lib.RECOMMEND_HELD_MAX_WIDTH, held_group.shape[1]))
    if held_len is not None and (not isinstance(held_len, torch.Tensor) or held_len.dim() != 1 or held_len.dtype != torch.int32):
        raise ValueError("held_len must be int32 [U]")
    # (picks and holdings together stay below 64 + 256: a cap beyond int32 never binds either)
    return cand_group, min(group_cap, (1 << 31) - 1), held_group, held_len


def _capped_dims(dims, cap):
    """``dims`` of ``_recommend_check`` with the length of ``cand_group`` held to the I it finds, and the held rows to U
    (``cap`` None: ``dims`` itself)."""
    if cap is None:
        return dims

    def capped(U, rows):
        I, n_t = dims(U, rows)
        if cap[0].shape[0] != I:
            raise ValueError("cand_group holds %d entries, the candidate list %d" % (cap[0].shape[0], I))
        if len(cap) > 2 and (cap[2].shape[0] != U or cap[3] is not None and cap[3].shape[0] != U):
            raise ValueError("held_group and held_len must hold one row per user (%d)" % U)
        return I, n_t
    return capped


def _cap_call(symbol, cap, dev):
    """(symbol, arguments, the tensors the arguments point into) of a capped launch behind item_ok: ``symbol`` + "_capped" with
    (cand_group, group_cap), or ``symbol`` + "_capped_held" with (held_group, held_len, held_stride) behind them - null
    pointers without a column."""
    group = cap[0].contiguous()
    args = (_lib.ptr(group), cap[1])
    if len(cap) == 2:
        return symbol + "_capped", args, (group,)
    held_group, held_len = cap[2], cap[3]
    W = int(held_group.shape[1])
    if W and held_len is None:
        held_len = torch.full((held_group.shape[0],), W, dtype=torch.int32, device=dev)
    rows = (held_group.contiguous(), held_len.contiguous()) if W else (None, None)
    return symbol + "_capped_held", args + (_lib.ptr(rows[0]), _lib.ptr(rows[1]), W), (group,) + rows


def recommend_topk(user_emb, item_emb, k, user_block=None, excl_pos=None, excl_len=None, item_ok=None, n_blocks=None, cand_group=None,
                   group_cap=None, held_group=None, held_len=None):
    """The k best candidates per user in one launch (``pfo_recommend_topk``); nothing but its outputs is written.

    user_emb f32[U,D]; item_emb f32[n_t*I,D]: n_t blocks of the same I candidates (embedded at n_t times); user_block
    i32[U] in [0,n_t): the block each user is scored against (None: one block).  ``n_blocks`` = n_t; when None it is 1 without
    ``user_block`` and rows / len(item_ok) with ``item_ok`` - with ``user_block`` alone it must be given.  score(u,i) =
    user_emb[u] . item_emb[user_block[u]*I + i] in fp32.  Candidate i is skipped for user u when ``item_ok[i] == 0`` (u8 / bool
    [I]) or when i occurs in ``excl_pos[u, :excl_len[u]]`` (i32[U,W] candidate POSITIONS, entries outside [0,I) ignored;
    excl_len i32[U], None: the whole row).

    Returns (top_pos i32[U,k], top_score f32[U,k], n_valid i32[U]): score descending, the larger position first among equal
    scores (the order of ``eval_metrics``); slots beyond the admissible candidates hold -1 / -inf.

    ``cand_group`` i32[I] with ``group_cap`` >= 1 (both or neither; ``pfo_recommend_topk_capped``): the list is the walk over
    that order that skips a candidate whose group - any non-negative id; negative: no group, never capped - holds ``group_cap``
    picks already.  Scores are the uncapped ones; n_valid counts what was taken.

    ``held_group`` i32[U,Wh] (at most 256 columns, padded with -1) with ``held_len`` i32[U] (None: the whole row), beside the
    cap pair (``pfo_recommend_topk_capped_held``): one group id per holding of the user; the count of a group starts from the
    entries of the row that name it, so a held name uses up quota and a group held ``group_cap`` times is closed from the
    start.  Negative entries count for nothing, an id named twice counts twice."""
    cap = _recommend_cap(cand_group, group_cap, held_group, held_len)
    dims = _capped_dims(_score_dims(n_blocks, item_ok, user_block), cap)
    user_emb, item_emb, user_block, excl_pos, excl_len, item_ok, U, D, k, I, n_t, W = _recommend_check(
        user_emb, item_emb, k, user_block, excl_pos, excl_len, item_ok, dims, cap[:1] + cap[2:] if cap else ())
    dev = user_emb.device
    top_pos = torch.empty((U, k), dtype=torch.int32, device=dev)
    top_score = torch.empty((U, k), dtype=torch.float32, device=dev)
    n_valid = torch.empty(U, dtype=torch.int32, device=dev)
    if cap is not None:
        symbol, cap_args, _alive = _cap_call("pfo_recommend_topk", cap, dev)
        _lib.call(symbol, user_emb.data_ptr(), item_emb.data_ptr(), _lib.ptr(user_block), U, I, n_t, D, _lib.ptr(excl_pos),
                  _lib.ptr(excl_len), W, _lib.ptr(item_ok), *cap_args, k, top_pos.data_ptr(), top_score.data_ptr(), n_valid.data_ptr(),
                  _lib.stream_ptr())
        return top_pos, top_score, n_valid
    _lib.call("pfo_recommend_topk", user_emb.data_ptr(), item_emb.data_ptr(), _lib.ptr(user_block), U, I, n_t, D, _lib.ptr(excl_pos),
              _lib.ptr(excl_len), W, _lib.ptr(item_ok), k, top_pos.data_ptr(), top_score.data_ptr(), n_valid.data_ptr(), _lib.stream_ptr())
    return top_pos, top_score, n_valid


_NO_WORKSPACE = object()     # ``_recommend_mv_launch``: the symbol takes no workspace (None: it does, allocate one)
_WIDE_WORKSPACE_CAP = 256 << 20


def _mv_dims(cand_stock, returns, day_idx, port_idx, port_len, n_blocks, max_items, then=None, port_w=None):
    """``dims`` of ``_recommend_check`` for the mean-variance forms: the checks of their own tensors, (I, n_t) from ``cand_stock``
    and ``n_blocks``.  ``max_items``: the form's bound on I; ``then(U, I)``: the caller's checks that need I, run behind it.
    ``port_w``: the weight rows of the weighted forms, f64 in the shape of ``port_idx``."""
    def dims(U, rows):
        if not isinstance(cand_stock, torch.Tensor) or cand_stock.dim() != 1 or cand_stock.dtype != torch.int32 or cand_stock.shape[0] < 1:
            raise ValueError("cand_stock must be int32 [I]")
        I = int(cand_stock.shape[0])
        if I > max_items:
            raise ValueError("%d candidates, at most %d with the mean-variance rank" % (I, max_items))
        if then is not None:
            then(U, I)
        n_t = 1 if n_blocks is None else int(n_blocks)
        if n_t < 1 or rows != n_t * I:
            raise ValueError("item_emb holds %d rows: not n_blocks = %d blocks of %d candidates" % (rows, n_t, I))
        if not isinstance(returns, torch.Tensor) or returns.dim() != 3 or returns.dtype != torch.float64 or 0 in returns.shape:
            raise ValueError("returns must be a float64 tensor [n_days, n_stocks, n_ret]")
        if not 2 <= returns.shape[2] <= 128:
            raise ValueError("n_ret must be in [2, 128] (got %d)" % returns.shape[2])
        if not isinstance(day_idx, torch.Tensor) or tuple(day_idx.shape) != (U,) or day_idx.dtype != torch.int32:
            raise ValueError("day_idx must be int32 [U]")
        if port_idx is not None:
            if port_idx.dim() != 2 or port_idx.shape[0] != U or port_idx.dtype != torch.int32:
                raise ValueError("port_idx must be int32 [U, W]")
            if port_len is not None and (tuple(port_len.shape) != (U,) or port_len.dtype != torch.int32):
                raise ValueError("port_len must be int32 [U]")
        elif port_len is not None:
            raise ValueError("port_len without port_idx")
        if port_w is not None:
            if port_idx is None:
                raise ValueError("port_w without port_idx: a weight weighs on a holding")
            if not isinstance(port_w, torch.Tensor) or port_w.dtype != torch.float64 or tuple(port_w.shape) != tuple(port_idx.shape):
                raise ValueError("port_w must be float64 [U, W], the shape of port_idx %s" % (tuple(port_idx.shape),))
        return I, n_t
    return dims


def _no_weights_with_cap(port_w, cand_group, group_cap):
    if port_w is not None and (cand_group is not None or group_cap is not None):
        raise ValueError("port_w and cand_group / group_cap cannot be combined: the capped orders have no weighted form")


def _recommend_mv_launch(symbol, diagnostics, user_emb, item_emb, k, cand_stock, returns, day_idx, port_idx, port_len, gamma, lambda_mv,
                         user_block, excl_pos, excl_len, item_ok, n_blocks, max_items=_lib.RECOMMEND_MV_MAX_ITEMS, workspace=_NO_WORKSPACE,
                         cap=None, port_w=None):
    """The argument checks, output rows and launch that ``recommend_mv_topk``, ``recommend_mv_topk_wide`` and
    ``recommend_basket_topk`` share: ``symbol`` takes pfo_recommend_mv_topk's arguments, with the three diagnostic arrays
    (``diagnostics``: allocate them or pass NULL) or without them (None).  ``max_items``: the symbol's bound on I.
    ``workspace``: for a symbol that takes (workspace, workspace_bytes) before the stream - a uint8 tensor, or None: allocated
    (what serves all users at once, 256 MiB at the most, the minimum at the least).  ``cap``: what ``_recommend_cap`` returns -
    with one, ``symbol`` + "_capped" (with held rows: + "_capped_held") is called, its arguments behind item_ok (``_cap_call``).
    ``port_w``: f64 [U, W] beside ``port_idx`` - ``symbol`` + "_weighted" is called, the rows behind port_len (never with ``cap``)."""
    def check_workspace(U, I):
        if workspace is not _NO_WORKSPACE and workspace is not None:
            if not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
                raise ValueError("workspace must be a contiguous uint8 tensor")
            if workspace.device != user_emb.device:
                raise ValueError("workspace lives on %s, the embeddings on %s" % (workspace.device, user_emb.device))
            need = _lib.byte_count("pfo_recommend_mv_wide_workspace_bytes", min(U, 16), I)
            if U and workspace.numel() < need:
                raise ValueError("workspace holds %d bytes, %d users of %d candidates need at least %d" % (workspace.numel(), U, I, need))
    dims = _capped_dims(_mv_dims(cand_stock, returns, day_idx, port_idx, port_len, n_blocks, max_items, check_workspace, port_w), cap)

    user_emb, item_emb, user_block, excl_pos, excl_len, item_ok, U, D, k, I, n_t, W = _recommend_check(
        user_emb, item_emb, k, user_block, excl_pos, excl_len, item_ok, dims,
        (cand_stock, returns, day_idx, port_idx, port_len, port_w) + (cap[:1] + cap[2:] if cap else ()))
    dev = user_emb.device
    n_days, n_stocks, n_ret = (int(v) for v in returns.shape)
    Wp = int(port_idx.shape[1]) if port_idx is not None else 0
    w_args = ()
    if port_w is not None:
        port_w = port_w.contiguous() if Wp else None
        symbol, w_args = symbol + "_weighted", (_lib.ptr(port_w),)
    if Wp and port_len is None:
        port_len = torch.full((U,), Wp, dtype=torch.int32, device=dev)
    top_pos = torch.empty((U, k), dtype=torch.int32, device=dev)
    top_score = torch.empty((U, k), dtype=torch.float32, device=dev)
    top_fused = torch.empty((U, k), dtype=torch.float64, device=dev)
    n_valid = torch.empty(U, dtype=torch.int32, device=dev)
    out = (top_pos, top_score, top_fused, n_valid)
    extra = ()
    if diagnostics is not None:
        extra = tuple(torch.empty((U, I), dtype=dt, device=dev) if diagnostics else None
                      for dt in (torch.float32, torch.float64, torch.float64))
    ws = ()
    if workspace is not _NO_WORKSPACE:
        if workspace is None:
            size = _lib.byte_count("pfo_recommend_mv_wide_workspace_bytes", U, I)
            size = max(min(size, _WIDE_WORKSPACE_CAP), _lib.byte_count("pfo_recommend_mv_wide_workspace_bytes", min(U, 16), I))
            workspace = torch.empty(size, dtype=torch.uint8, device=dev)
        ws = (workspace.data_ptr(), workspace.numel())
    cap_args = ()
    if cap is not None:
        symbol, cap_args, _alive = _cap_call(symbol, cap, dev)
    _lib.call(symbol, user_emb.data_ptr(), item_emb.data_ptr(), _lib.ptr(user_block), U, I, n_t, D, _lib.ptr(excl_pos), _lib.ptr(excl_len),
              W, _lib.ptr(item_ok), *cap_args, _lib.ptr(cand_stock.contiguous()), returns.contiguous().data_ptr(), n_days, n_stocks, n_ret,
              _lib.ptr(day_idx.contiguous()), _lib.ptr(port_idx.contiguous() if Wp else None), _lib.ptr(port_len.contiguous() if Wp else None),
              *w_args, Wp, float(gamma), float(lambda_mv), k, *(t.data_ptr() for t in out), *(_lib.ptr(t) for t in extra), *ws,
              _lib.stream_ptr())
    return out + extra if diagnostics else out


def recommend_mv_topk(user_emb, item_emb, k, cand_stock, returns, day_idx, port_idx, port_len, gamma, lambda_mv, user_block=None,
                      excl_pos=None, excl_len=None, item_ok=None, n_blocks=None, want_all=False, port_w=None, cand_group=None,
                      group_cap=None, held_group=None, held_len=None):
    """``recommend_topk`` with the mean-variance rank fusion of main.py:243-289 over every user's whole candidate list, in one
    launch (``pfo_recommend_mv_topk``).

    The arguments of ``recommend_topk`` mean what they mean there and the score is that kernel's to the bit.  cand_stock
    i32[I]: row of candidate i in ``returns`` f64[n_days,n_stocks,n_ret] (``MVSampler.returns``); day_idx i32[U]; port_idx
    i32[U,W], port_len i32[U] (None: whole rows): the stock rows user u holds, entries outside [0,n_stocks) ignored,
    duplicates counted.  Over the admissible candidates of a user (the rules of ``recommend_topk``, minus cand_stock outside the
    table, minus a NaN y; none for a day outside the table): fused = lambda_mv * rank(y_mv) + (1 - lambda_mv) * rank(score), both
    average-tie ranks (``scipy.stats.rankdata``).

    Returns (top_pos i32[U,k], top_score f32[U,k], top_fused f64[U,k], n_valid i32[U]): fused descending, the larger position
    first among equal values; empty slots -1 / -inf / -inf.  ``want_all`` adds (score f32[U,I], y f64[U,I],
    fused f64[U,I]), NaN in the last two where a candidate is not admissible.

    ``cand_group`` i32[I] with ``group_cap`` >= 1 (both or neither; ``pfo_recommend_mv_topk_capped``): the walk over that order
    skips a candidate whose group (negative: none) holds ``group_cap`` picks already.  Ranks, fused and the ``want_all`` arrays
    are the uncapped ones - a cap changes no rank.  ``held_group`` / ``held_len`` beside them (``recommend_topk`` describes the
    rows; ``pfo_recommend_mv_topk_capped_held``): the count of a group starts from what the user holds of it.

    ``port_w`` f64[U,W] on the device, the shape of ``port_idx`` (``pfo_recommend_mv_topk_weighted``): holding p weighs
    ``port_w[u, p]`` on y in place of 1 / n_holding - ``(1 / sum w) * sum(w * cov)`` over the holdings whose stock is in the
    table and whose weight is finite and > 0; the others are left out.  All-ones rows give the unweighted result bit for bit.
    None takes the unweighted path; with ``cand_group`` a ValueError (the capped orders have no weighted form)."""
    _no_weights_with_cap(port_w, cand_group, group_cap)
    return _recommend_mv_launch("pfo_recommend_mv_topk", bool(want_all), user_emb, item_emb, k, cand_stock, returns, day_idx, port_idx,
                                port_len, gamma, lambda_mv, user_block, excl_pos, excl_len, item_ok, n_blocks,
                                cap=_recommend_cap(cand_group, group_cap, held_group, held_len), port_w=port_w)


def recommend_mv_topk_wide(user_emb, item_emb, k, cand_stock, returns, day_idx, port_idx, port_len, gamma, lambda_mv, user_block=None,
                           excl_pos=None, excl_len=None, item_ok=None, n_blocks=None, workspace=None, want_all=False, port_w=None):
    """``recommend_mv_topk`` for candidate lists beyond its 2048 (``pfo_recommend_mv_topk_wide``, up to 65536): the same
    arguments, checks and return tuple, the same results to the bit where both apply.  The state of a user lives in
    ``workspace`` and the ranks are found by sorting, O(I log I) per user.

    ``workspace``: a contiguous uint8 tensor on the embeddings' device of at least
    ``pfo_recommend_mv_wide_workspace_bytes(min(U, 16), I)`` bytes (36 bytes per user and candidate, users in tiles of 16,
    candidates rounded up to 16); the users are served in slabs of as many tiles as it holds, and the result does not depend on
    its size.  None: allocated - what serves all users at once, 256 MiB at the most.

    ``port_w`` f64[U,W]: the weight rows of ``recommend_mv_topk`` (``pfo_recommend_mv_topk_wide_weighted``)."""
    return _recommend_mv_launch("pfo_recommend_mv_topk_wide", bool(want_all), user_emb, item_emb, k, cand_stock, returns, day_idx,
                                port_idx, port_len, gamma, lambda_mv, user_block, excl_pos, excl_len, item_ok, n_blocks,
                                _lib.RECOMMEND_MV_WIDE_MAX_ITEMS, workspace, port_w=port_w)


def recommend_basket_topk(user_emb, item_emb, k, cand_stock, returns, day_idx, port_idx, port_len, gamma, lambda_mv, user_block=None,
                          excl_pos=None, excl_len=None, item_ok=None, n_blocks=None, cand_group=None, group_cap=None, held_group=None,
                          held_len=None):
    """``recommend_mv_topk`` taken one pick at a time, in one launch (``pfo_recommend_basket_topk``): pick r is the first of the
    canonical order of round r, in which the stocks of picks 0 .. r-1 count as held behind ``port_idx[u]`` (in pick order) and
    their positions have left the pool; only the position leaves - another candidate on the same stock stays.  Arguments and
    their checks are ``recommend_mv_topk``'s.

    Returns (top_pos i32[U,k], top_score f32[U,k], top_fused f64[U,k], n_valid i32[U]): ``top_fused[u, r]`` is the pick's fused
    value OF ROUND r (a row need not descend); the list ends when no candidate is left, empty slots -1 / -inf / -inf.  k = 1 is
    ``recommend_mv_topk`` bit for bit; any k equals k calls of it with k = 1, each pick appended to the user's portfolio row and
    exclusion row.

    ``cand_group`` i32[I] with ``group_cap`` >= 1 (both or neither; ``pfo_recommend_basket_topk_capped``): a group (negative:
    none) that holds ``group_cap`` picks leaves the pool - its candidates take part in no later round, like excluded ones.  Any
    k then equals the k = 1 loop above with every other candidate of a full group appended to the exclusion row as well.
    ``held_group`` / ``held_len`` beside them (``recommend_topk`` describes the rows; ``pfo_recommend_basket_topk_capped_held``):
    a group is full at picks + holdings >= ``group_cap``, and one that the holdings alone fill is out of the pool of round 0 too."""
    return _recommend_mv_launch("pfo_recommend_basket_topk", None, user_emb, item_emb, k, cand_stock, returns, day_idx, port_idx,
                                port_len, gamma, lambda_mv, user_block, excl_pos, excl_len, item_ok, n_blocks,
                                cap=_recommend_cap(cand_group, group_cap, held_group, held_len))


def _recommend_list_check(user_emb, item_emb, k, list_pos, list_len, user_block, item_ok, dims, also=()):
    """``_recommend_check`` for the list forms: the list pair in place of the exclusion pair (it takes the same checks, under
    its own names), at least one and at most ``RECOMMEND_LIST_MAX_WIDTH`` columns.  Returns what ``_recommend_check`` returns."""
    if not isinstance(list_pos, torch.Tensor) or list_pos.dim() != 2 or list_pos.dtype != torch.int32 or list_pos.shape[0] != user_emb.shape[0]:
        raise ValueError("list_pos must be int32 [U, W]")
    if not 1 <= list_pos.shape[1] <= _lib.RECOMMEND_LIST_MAX_WIDTH:
        raise ValueError("list_pos must have between 1 and %d columns (got %d)" % (_lib.RECOMMEND_LIST_MAX_WIDTH, list_pos.shape[1]))
    if list_len is not None and (not isinstance(list_len, torch.Tensor) or list_len.dim() != 1 or list_len.shape[0] != list_pos.shape[0]
                                 or list_len.dtype != torch.int32):
        raise ValueError("list_len must be int32 [U]")
    return _recommend_check(user_emb, item_emb, k, user_block, list_pos, list_len, item_ok, dims, also)


def recommend_list_topk(user_emb, item_emb, k, list_pos, list_len, user_block=None, item_ok=None, n_blocks=None, want_all=False):
    """The k best of every user's OWN list in one launch (``pfo_recommend_list_topk``): ``recommend_topk`` with
    ``list_pos`` i32[U,W] (1 <= W <= 256) / ``list_len`` i32[U] (None: whole rows) naming the candidate POSITIONS user u may be
    offered, in place of an exclusion list.  Entries outside [0,I) are ignored, a position named more than once counts once, an
    empty list gives an empty answer; ``item_ok`` still removes candidates.  The other arguments and their checks are
    ``recommend_topk``'s; the users need not be sorted by block, and I is bounded by 65536 alone.

    The score is an fp32 dot product within the any-order error bound - not ``recommend_topk``'s bits (another summation order).

    Returns (top_pos i32[U,k], top_score f32[U,k], n_valid i32[U]) as ``recommend_topk`` does.  ``want_all`` adds score
    f32[U,W] BY LIST SLOT, NaN in every slot that is not the first occurrence of an admissible position."""
    dims = _score_dims(n_blocks, item_ok, user_block)
    user_emb, item_emb, user_block, list_pos, list_len, item_ok, U, D, k, I, n_t, W = _recommend_list_check(
        user_emb, item_emb, k, list_pos, list_len, user_block, item_ok, dims)
    dev = user_emb.device
    top_pos = torch.empty((U, k), dtype=torch.int32, device=dev)
    top_score = torch.empty((U, k), dtype=torch.float32, device=dev)
    n_valid = torch.empty(U, dtype=torch.int32, device=dev)
    score = torch.empty((U, W), dtype=torch.float32, device=dev) if want_all else None
    _lib.call("pfo_recommend_list_topk", user_emb.data_ptr(), item_emb.data_ptr(), _lib.ptr(user_block), U, I, n_t, D, _lib.ptr(list_pos),
              _lib.ptr(list_len), W, _lib.ptr(item_ok), k, top_pos.data_ptr(), top_score.data_ptr(), n_valid.data_ptr(), _lib.ptr(score),
              _lib.stream_ptr())
    return (top_pos, top_score, n_valid, score) if want_all else (top_pos, top_score, n_valid)


def recommend_list_mv_topk(user_emb, item_emb, k, list_pos, list_len, cand_stock, returns, day_idx, port_idx, port_len, gamma, lambda_mv,
                           user_block=None, item_ok=None, n_blocks=None, want_all=False, port_w=None):
    """``recommend_list_topk`` in the mean-variance order (``pfo_recommend_list_mv_topk``): the rank fusion of
    ``recommend_mv_topk`` - its arguments, its y, its average-tie ranks, its blend - over every user's own list.  A listed
    candidate must also have a y (day and ``cand_stock`` inside the tables, y not NaN).  No bound of 2048 on I and no workspace:
    only the list, 256 entries at the most, is ranked.  The portfolio is used as given - a list of the user's own holdings is
    ranked against those holdings, itself among them.  At ``lambda_mv = 0`` positions and scores are ``recommend_list_topk``'s
    bit for bit where every listed candidate has a y.

    Returns (top_pos i32[U,k], top_score f32[U,k], top_fused f64[U,k], n_valid i32[U]); ``want_all`` adds (score f32[U,W],
    y f64[U,W], fused f64[U,W]) BY LIST SLOT, NaN in every slot that is not the first occurrence of an admissible position.

    ``port_w`` f64[U,Wp], the shape of ``port_idx``: the weight rows of ``recommend_mv_topk``
    (``pfo_recommend_list_mv_topk_weighted``)."""
    dims = _mv_dims(cand_stock, returns, day_idx, port_idx, port_len, n_blocks, _lib.RECOMMEND_MAX_ITEMS, port_w=port_w)
    user_emb, item_emb, user_block, list_pos, list_len, item_ok, U, D, k, I, n_t, W = _recommend_list_check(
        user_emb, item_emb, k, list_pos, list_len, user_block, item_ok, dims, (cand_stock, returns, day_idx, port_idx, port_len, port_w))
    dev = user_emb.device
    n_days, n_stocks, n_ret = (int(v) for v in returns.shape)
    Wp = int(port_idx.shape[1]) if port_idx is not None else 0
    if Wp and port_len is None:
        port_len = torch.full((U,), Wp, dtype=torch.int32, device=dev)
    out = (torch.empty((U, k), dtype=torch.int32, device=dev), torch.empty((U, k), dtype=torch.float32, device=dev),
           torch.empty((U, k), dtype=torch.float64, device=dev), torch.empty(U, dtype=torch.int32, device=dev))
    extra = tuple(torch.empty((U, W), dtype=dt, device=dev) if want_all else None for dt in (torch.float32, torch.float64, torch.float64))
    symbol, w_args = "pfo_recommend_list_mv_topk", ()
    if port_w is not None:
        port_w = port_w.contiguous() if Wp else None
        symbol, w_args = symbol + "_weighted", (_lib.ptr(port_w),)
    _lib.call(symbol, user_emb.data_ptr(), item_emb.data_ptr(), _lib.ptr(user_block), U, I, n_t, D, _lib.ptr(list_pos),
              _lib.ptr(list_len), W, _lib.ptr(item_ok), _lib.ptr(cand_stock.contiguous()), returns.contiguous().data_ptr(), n_days, n_stocks,
              n_ret, _lib.ptr(day_idx.contiguous()), _lib.ptr(port_idx.contiguous() if Wp else None),
              _lib.ptr(port_len.contiguous() if Wp else None), *w_args, Wp, float(gamma), float(lambda_mv), k, *(t.data_ptr() for t in out),
              *(_lib.ptr(t) for t in extra), _lib.stream_ptr())
    return out + extra if want_all else out


def holdings_store(src, port_idx, port_len, ts, hold_idx, hold_len, hold_time, scratch=None):
    """Writes the ledger rows of the events' users in place (``pfo_holdings_store``): for every event in input order, users
    outside [1, n_nodes) skipped, ``hold_idx[u] = port_idx[e, :L]`` padded with -1, ``hold_len[u] = L`` =
    clamp(port_len[e], 0, min(W, Wp)), ``hold_time[u] = ts[e]``; per user the last event wins.

    src i32[N], port_idx i32[N, Wp], port_len i32[N], ts f64[N]; hold_idx i32[n_nodes, W], hold_len i32[n_nodes], hold_time
    f64[n_nodes] contiguous; scratch: a uint8 / int32 tensor of ``pfo_holdings_store_scratch_bytes`` bytes or None (allocated)."""
    if (hold_idx.dim() != 2 or hold_idx.dtype != torch.int32 or hold_len.dtype != torch.int32 or hold_time.dtype != torch.float64
            or tuple(hold_len.shape) != (hold_idx.shape[0],) or tuple(hold_time.shape) != (hold_idx.shape[0],)):
        raise ValueError("the ledger must be (i32 [n_nodes, W], i32 [n_nodes], f64 [n_nodes])")
    if not (hold_idx.is_contiguous() and hold_len.is_contiguous() and hold_time.is_contiguous()):
        raise ValueError("the ledger tables must be contiguous")
    n_nodes, W = (int(v) for v in hold_idx.shape)
    N = int(src.shape[0]) if src.dim() == 1 else -1
    if (src.dtype != torch.int32 or N < 0 or port_idx.dim() != 2 or port_idx.dtype != torch.int32 or port_idx.shape[0] != N
            or port_len.dtype != torch.int32 or tuple(port_len.shape) != (N,) or ts.dtype != torch.float64 or tuple(ts.shape) != (N,)):
        raise ValueError("events must be src i32[N], port_idx i32[N, Wp], port_len i32[N], ts f64[N]")
    dev = hold_idx.device
    _lib.require_gpu(dev)
    for t in (src, port_idx, port_len, ts, hold_len, hold_time, scratch):
        if t is not None and t.device != dev:
            raise ValueError("all tensors must live on %s" % dev)
    need = _lib.byte_count("pfo_holdings_store_scratch_bytes", n_nodes, N)
    if scratch is None or scratch.numel() * scratch.element_size() < need or not scratch.is_contiguous():
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    Wp = int(port_idx.shape[1])
    _lib.call("pfo_holdings_store", _lib.ptr(src.contiguous()), _lib.ptr(port_idx.contiguous() if Wp else None),
              _lib.ptr(port_len.contiguous()), Wp, _lib.ptr(ts.contiguous()), N, hold_idx.data_ptr(), hold_len.data_ptr(),
              hold_time.data_ptr(), n_nodes, W, scratch.data_ptr(), scratch.numel() * scratch.element_size(), _lib.stream_ptr())


def holdings_apply(src, stock, side, ts, hold_idx, hold_len, hold_time, qty=None, hold_qty=None, counters=None, scratch=None):
    """Applies buys and sells to the ledger rows in place, in event order (``pfo_holdings_apply``; the rules are stated in
    include/pfotgn.h): a buy appends the stock behind the row's live entries or adds to its share count, a sell takes from the
    count or closes the position - the entries behind it move one slot to the front -, every valid event sets the row's time.
    Invalid events (user outside [1, n_nodes), negative stock, a side that is not +1 / -1, with both ``hold_qty`` and ``qty`` a
    quantity that is not finite and positive) are skipped whole.

    src / stock / side i32[N], ts f64[N], qty f64[N] or None (every quantity 1.0; ignored without ``hold_qty``); hold_idx
    i32[n_nodes, W], hold_len i32[n_nodes], hold_time f64[n_nodes], hold_qty f64[n_nodes, W] or None, all contiguous; counters:
    int64[2] (overflow: buys into a full row; unmatched: sells of a stock the row does not hold) the call ADDS to, or None;
    scratch: a uint8 / int32 tensor of ``pfo_holdings_apply_scratch_bytes`` bytes or None (allocated)."""
    if (hold_idx.dim() != 2 or hold_idx.dtype != torch.int32 or hold_len.dtype != torch.int32 or hold_time.dtype != torch.float64
            or tuple(hold_len.shape) != (hold_idx.shape[0],) or tuple(hold_time.shape) != (hold_idx.shape[0],)):
        raise ValueError("the ledger must be (i32 [n_nodes, W], i32 [n_nodes], f64 [n_nodes])")
    if hold_qty is not None and (hold_qty.dtype != torch.float64 or tuple(hold_qty.shape) != tuple(hold_idx.shape)):
        raise ValueError("the ledger's quantities must be f64 [n_nodes, W]")
    if not all(t is None or t.is_contiguous() for t in (hold_idx, hold_len, hold_time, hold_qty, counters)):
        raise ValueError("the ledger tables must be contiguous")
    if counters is not None and (counters.dtype != torch.int64 or tuple(counters.shape) != (2,)):
        raise ValueError("counters must be int64 [2]")
    n_nodes, W = (int(v) for v in hold_idx.shape)
    N = int(src.shape[0]) if src.dim() == 1 else -1
    if (N < 0 or any(t.dtype != torch.int32 or tuple(t.shape) != (N,) for t in (src, stock, side)) or ts.dtype != torch.float64
            or tuple(ts.shape) != (N,) or (qty is not None and (qty.dtype != torch.float64 or tuple(qty.shape) != (N,)))):
        raise ValueError("events must be src i32[N], stock i32[N], side i32[N], ts f64[N] and qty f64[N] or None")
    dev = hold_idx.device
    _lib.require_gpu(dev)
    for t in (src, stock, side, ts, qty, hold_len, hold_time, hold_qty, counters, scratch):
        if t is not None and t.device != dev:
            raise ValueError("all tensors must live on %s" % dev)
    need = _lib.byte_count("pfo_holdings_apply_scratch_bytes", n_nodes, N)
    if scratch is None or scratch.numel() * scratch.element_size() < need or not scratch.is_contiguous():
        scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    _lib.call("pfo_holdings_apply", _lib.ptr(src.contiguous()), _lib.ptr(stock.contiguous()), _lib.ptr(side.contiguous()),
              _lib.ptr(qty.contiguous() if qty is not None else None), _lib.ptr(ts.contiguous()), N, hold_idx.data_ptr(),
              hold_len.data_ptr(), hold_time.data_ptr(), _lib.ptr(hold_qty), n_nodes, W, _lib.ptr(counters), scratch.data_ptr(),
              scratch.numel() * scratch.element_size(), _lib.stream_ptr())


def holdings_gather(users, hold_idx, hold_len, upper_u, items=None, pos_scratch=None):
    """The ledger rows of ``users`` i32[U] (``pfo_holdings_gather``): (port_idx i32[U, W], port_len i32[U], excl_pos) - users
    outside [0, n_nodes) give (-1.., 0).  With ``items`` i32[I] (distinct candidate node ids) excl_pos i32[U, W] holds, per
    valid entry, the position in ``items`` of node ``stock + upper_u + 1`` or -1; without, None.  ``pos_scratch``: i32[>= n_nodes]
    kept between queries (any content), None: allocated."""
    if hold_idx.dim() != 2 or hold_idx.dtype != torch.int32 or hold_len.dtype != torch.int32 or tuple(hold_len.shape) != (hold_idx.shape[0],):
        raise ValueError("the ledger must be (i32 [n_nodes, W], i32 [n_nodes])")
    if not (hold_idx.is_contiguous() and hold_len.is_contiguous()):
        raise ValueError("the ledger tables must be contiguous")
    if users.dim() != 1 or users.dtype != torch.int32:
        raise ValueError("users must be int32 [U]")
    n_nodes, W = (int(v) for v in hold_idx.shape)
    U, I = int(users.shape[0]), 1
    dev = hold_idx.device
    if items is not None:
        if items.dim() != 1 or items.dtype != torch.int32:
            raise ValueError("items must be int32 [I]")
        I = int(items.shape[0])
        if pos_scratch is None or pos_scratch.dtype != torch.int32 or pos_scratch.numel() < n_nodes or not pos_scratch.is_contiguous():
            pos_scratch = torch.empty(n_nodes, dtype=torch.int32, device=dev)
    _lib.require_gpu(dev)
    for t in (users, hold_len, items, pos_scratch if items is not None else None):
        if t is not None and t.device != dev:
            raise ValueError("all tensors must live on %s" % dev)
    port_idx = torch.empty((U, W), dtype=torch.int32, device=dev)
    port_len = torch.empty(U, dtype=torch.int32, device=dev)
    excl_pos = torch.empty((U, W), dtype=torch.int32, device=dev) if items is not None else None
    _lib.call("pfo_holdings_gather", _lib.ptr(users.contiguous()), U, hold_idx.data_ptr(), hold_len.data_ptr(), n_nodes, W,
              _lib.ptr(items.contiguous() if items is not None else None), I, int(upper_u),
              _lib.ptr(pos_scratch if items is not None else None), port_idx.data_ptr(), port_len.data_ptr(), _lib.ptr(excl_pos),
              _lib.stream_ptr())
    return port_idx, port_len, excl_pos


WEIGHT_MODES = {"shares": 0, "value": 1}


def holdings_gather_weights(users, hold_idx, hold_len, hold_qty, mode, last_close=None):
    """The weight rows of ``users`` i32[U] beside ``holdings_gather``'s port_idx (``pfo_holdings_gather_weights``): f64[U, W],
    0.0 at and behind the row's length and for users outside [0, n_nodes).  ``mode`` "shares" (or 0): the share counts
    ``hold_qty[u, j]``; "value" (or 1): share count x ``last_close[stock]`` f64[n_stocks] (one rounded product), 0.0 for a stock
    outside the table, NaN for a stock never quoted - ``recommend_mv_topk`` leaves both out.  One launch, every slot written."""
    mode = WEIGHT_MODES.get(mode, mode) if isinstance(mode, str) else mode
    if mode not in (0, 1) or isinstance(mode, bool):
        raise ValueError('mode must be "shares" (0) or "value" (1)')
    if hold_idx.dim() != 2 or hold_idx.dtype != torch.int32 or hold_len.dtype != torch.int32 or tuple(hold_len.shape) != (hold_idx.shape[0],):
        raise ValueError("the ledger must be (i32 [n_nodes, W], i32 [n_nodes])")
    if not isinstance(hold_qty, torch.Tensor) or hold_qty.dtype != torch.float64 or tuple(hold_qty.shape) != tuple(hold_idx.shape):
        raise ValueError("the ledger's quantities must be f64 [n_nodes, W]: the weights are share counts")
    if not (hold_idx.is_contiguous() and hold_len.is_contiguous() and hold_qty.is_contiguous()):
        raise ValueError("the ledger tables must be contiguous")
    if users.dim() != 1 or users.dtype != torch.int32:
        raise ValueError("users must be int32 [U]")
    n_stocks = 0
    if mode == 1:
        if not isinstance(last_close, torch.Tensor) or last_close.dim() != 1 or last_close.dtype != torch.float64:
            raise ValueError('mode "value" needs last_close f64 [n_stocks]')
        n_stocks = int(last_close.shape[0])
    n_nodes, W = (int(v) for v in hold_idx.shape)
    U = int(users.shape[0])
    dev = hold_idx.device
    _lib.require_gpu(dev)
    for t in (users, hold_len, hold_qty, last_close if mode == 1 else None):
        if t is not None and t.device != dev:
            raise ValueError("all tensors must live on %s" % dev)
    w_out = torch.empty((U, W), dtype=torch.float64, device=dev)
    _lib.call("pfo_holdings_gather_weights", _lib.ptr(users.contiguous()), U, hold_idx.data_ptr(), hold_len.data_ptr(), hold_qty.data_ptr(),
              n_nodes, W, _lib.ptr(last_close.contiguous() if mode == 1 else None), n_stocks, mode, w_out.data_ptr(), _lib.stream_ptr())
    return w_out


HISTORY_OUTPUTS = ("node", "len", "time", "count", "pos", "stock")


def history_gather(indptr, adj_nbr, adj_ts, users, ts, width, since=None, max_scan=0, items=None, pos_scratch=None, upper_u=None,
                   want=("node", "len", "time", "count")):
    """What each user has interacted with before its time, from a finder's device CSR (``pfo_history_gather``; the semantics
    are stated in include/pfotgn.h): per query the distinct neighbours of row ``users[q]`` among the entries with
    ``since[q] <= adj_ts < ts[q]`` (fp64, strict at the top), newest first, at most ``width`` of them; ``max_scan`` > 0 looks at
    the newest ``max_scan`` entries of that window only.  Returns the tensors ``want`` names, in its order:

    node i32[U, W] padded with -1, len i32[U], time f64[U, W] (the newest timestamp of each kept neighbour, NaN padding), count
    i32[U, W] (the window's entries that name it, once the list is full the walk goes on for the counts alone), pos i32[U, W]
    (position in ``items`` i32[I], distinct node ids, -1 for a non-candidate; ``pos_scratch``: contiguous i32[>= n_nodes] kept
    between queries with any content - anything else is refused, never replaced -, None: allocated), stock i32[U, W] (node - ``upper_u`` - 1, -1 outside [0, 2^31)).

    indptr i64[n_nodes + 1], adj_nbr i32, adj_ts f64 as ``NeighborFinder.device_arrays`` returns them; users i32[U], ts f64[U],
    since f64[U] or None (a NaN entry: no lower end for that user).  ValueError: what the C entry refuses."""
    try:
        want = tuple(want)
    except TypeError:
        raise ValueError("want must name outputs among %s" % (HISTORY_OUTPUTS,)) from None
    if any(w not in HISTORY_OUTPUTS for w in want):
        raise ValueError("want must name outputs among %s, got %s" % (HISTORY_OUTPUTS, want))
    try:
        W, max_scan = int(width), int(max_scan)
    except (TypeError, ValueError):
        raise ValueError("width and max_scan must be integers") from None
    if not 1 <= W <= _lib.HISTORY_MAX_WIDTH:
        raise ValueError("width must lie in [1, %d] (got %d)" % (_lib.HISTORY_MAX_WIDTH, W))
    if max_scan < 0:
        raise ValueError("max_scan must not be negative (got %d)" % max_scan)
    if indptr.dim() != 1 or indptr.dtype != torch.int64 or indptr.shape[0] < 2 or indptr.shape[0] - 1 >= 2 ** 31:
        raise ValueError("indptr must be int64 [n_nodes + 1] with 1 <= n_nodes < 2^31")
    if adj_nbr.dtype != torch.int32 or adj_ts.dtype != torch.float64 or adj_nbr.dim() != 1 or adj_nbr.shape != adj_ts.shape:
        raise ValueError("the adjacency must be adj_nbr i32[n] next to adj_ts f64[n]")
    if not (indptr.is_contiguous() and adj_nbr.is_contiguous() and adj_ts.is_contiguous()):
        raise ValueError("the adjacency arrays must be contiguous")
    if users.dim() != 1 or users.dtype != torch.int32:
        raise ValueError("users must be int32 [U]")
    U, n_nodes, I = int(users.shape[0]), int(indptr.shape[0]) - 1, 1
    if ts.dtype != torch.float64 or tuple(ts.shape) != (U,):
        raise ValueError("ts must be float64 [U] (U = %d)" % U)
    if since is not None and (since.dtype != torch.float64 or tuple(since.shape) != (U,)):
        raise ValueError("since must be float64 [U] (U = %d) or None" % U)
    dev = indptr.device
    if "pos" in want:
        if items is None or items.dim() != 1 or items.dtype != torch.int32:
            raise ValueError("positions need items: int32 [I]")
        I = int(items.shape[0])
        if not 1 <= I <= _lib.RECOMMEND_MAX_ITEMS:
            raise ValueError("items must hold between 1 and %d candidates (got %d)" % (_lib.RECOMMEND_MAX_ITEMS, I))
        if pos_scratch is None:
            pos_scratch = torch.empty(n_nodes, dtype=torch.int32, device=dev)
        elif pos_scratch.dtype != torch.int32 or pos_scratch.numel() < n_nodes or not pos_scratch.is_contiguous():
            raise ValueError("pos_scratch must be a contiguous int32 tensor of at least n_nodes = %d entries (or None)" % n_nodes)
    else:
        items = pos_scratch = None
    if "stock" in want:
        if upper_u is None or not 0 <= int(upper_u) < 2 ** 31 - 1:
            raise ValueError("stock indices need upper_u: a non-negative int32")
    _lib.require_gpu(dev)
    for t in (adj_nbr, adj_ts, users, ts, since, items, pos_scratch):
        if t is not None and t.device != dev:
            raise ValueError("all tensors must live on %s" % dev)
    out = dict(node=torch.empty((U, W), dtype=torch.int32, device=dev), len=torch.empty(U, dtype=torch.int32, device=dev))
    for name, dt in (("time", torch.float64), ("count", torch.int32), ("pos", torch.int32), ("stock", torch.int32)):
        out[name] = torch.empty((U, W), dtype=dt, device=dev) if name in want else None
    _lib.call("pfo_history_gather", indptr.data_ptr(), _lib.ptr(adj_nbr), _lib.ptr(adj_ts), n_nodes, _lib.ptr(users.contiguous()),
              _lib.ptr(ts.contiguous()), _lib.ptr(None if since is None else since.contiguous()), U, W, max_scan,
              _lib.ptr(None if items is None else items.contiguous()), I, _lib.ptr(pos_scratch), int(upper_u or 0),
              out["node"].data_ptr(), out["len"].data_ptr(), _lib.ptr(out["time"]), _lib.ptr(out["count"]), _lib.ptr(out["pos"]),
              _lib.ptr(out["stock"]), _lib.stream_ptr())
    return tuple(out[w] for w in want)


def returns_scatter_closes(stocks, closes, n_stocks, stamp=None):
    """The sparse form of a day's closes -> the stamp table ``pfo_returns_append_day`` reads (``pfo_returns_scatter_closes``: a
    memset and one launch).  stocks i32[m], closes f64[m]; positions whose index lies outside [0, n_stocks) or whose close is
    not positive and finite are skipped, among repeated indices the last valid position wins.  ``stamp``: i32[>= n_stocks]
    kept between calls (any content), None: allocated.  Returns the stamp tensor."""
    m = int(stocks.shape[0]) if stocks.dim() == 1 else -1
    if stocks.dtype != torch.int32 or m < 0 or closes.dtype != torch.float64 or tuple(closes.shape) != (m,):
        raise ValueError("sparse closes must be stocks i32[m] next to closes f64[m]")
    dev = closes.device
    _lib.require_gpu(dev)
    n_stocks = int(n_stocks)
    if stamp is None or stamp.dtype != torch.int32 or stamp.numel() < n_stocks or not stamp.is_contiguous():
        stamp = torch.empty(max(n_stocks, 1), dtype=torch.int32, device=dev)
    if stocks.device != dev or stamp.device != dev:
        raise ValueError("all tensors must live on %s" % dev)
    _lib.call("pfo_returns_scatter_closes", _lib.ptr(stocks.contiguous()), _lib.ptr(closes.contiguous()), m, n_stocks, stamp.data_ptr(),
              stamp.numel() * 4, _lib.stream_ptr())
    return stamp


def returns_append_day(returns, day_keys, last_close, prev_slot, new_slot, n_stocks, day_key, closes, stamp=None, want_quotients=False):
    """One trading day appended to a return table in place (``pfo_returns_append_day``, one launch): rows [0, n_stocks) of slot
    ``new_slot`` of ``returns`` f64[day_cap, stock_cap, n_ret] become the rows of ``prev_slot`` shifted by one with the newest
    return ``log(close / last_close)`` (+0 for a stock not quoted today or never quoted before) in the last column;
    ``day_keys[new_slot] = day_key``; ``last_close`` f64[>= n_stocks] takes today's closes where quoted.  ``prev_slot`` -1: the
    first day, all zeros.  closes f64[n]: dense (entry s is stock s, NaN = not quoted), or with ``stamp`` (the table
    ``returns_scatter_closes`` made of the sparse form) the closes that table points into.  ``want_quotients``: returns
    f64[n_stocks], the quotient each logarithm was taken of (NaN where none was) - for tests."""
    if (not isinstance(returns, torch.Tensor) or returns.dim() != 3 or returns.dtype != torch.float64 or not returns.is_contiguous()
            or 0 in returns.shape):
        raise ValueError("returns must be a contiguous float64 tensor [day_cap, stock_cap, n_ret]")
    day_cap, stock_cap, n_ret = (int(v) for v in returns.shape)
    if day_keys.dtype != torch.int64 or tuple(day_keys.shape) != (day_cap,) or not day_keys.is_contiguous():
        raise ValueError("day_keys must be a contiguous int64 tensor [day_cap]")
    n_stocks = int(n_stocks)
    if last_close.dtype != torch.float64 or last_close.dim() != 1 or last_close.shape[0] < n_stocks or not last_close.is_contiguous():
        raise ValueError("last_close must be a contiguous float64 tensor of at least n_stocks entries")
    if closes.dtype != torch.float64 or closes.dim() != 1:
        raise ValueError("closes must be float64 [n]")
    if stamp is not None and (stamp.dtype != torch.int32 or stamp.numel() < n_stocks or not stamp.is_contiguous()):
        raise ValueError("stamp must be a contiguous int32 tensor of at least n_stocks entries")
    dev = returns.device
    _lib.require_gpu(dev)
    for t in (day_keys, last_close, closes, stamp):
        if t is not None and t.device != dev:
            raise ValueError("all tensors must live on %s" % dev)
    quot = torch.empty(n_stocks, dtype=torch.float64, device=dev) if want_quotients else None
    n = int(closes.shape[0])
    _lib.call("pfo_returns_append_day", returns.data_ptr(), day_cap, stock_cap, n_ret, int(prev_slot), int(new_slot), n_stocks,
              _lib.ptr(closes.contiguous() if n else None), n, _lib.ptr(stamp), last_close.data_ptr(), day_keys.data_ptr(), int(day_key),
              _lib.ptr(quot), _lib.stream_ptr())
    return quot


def day_lookup(ts, day_keys, head, n_days, key_divisor):
    """slot i32[U] of the live day each timestamp falls on (``pfo_day_lookup``, one launch): key = (int64) floor(ts / key_divisor)
    searched among the ``n_days`` live slots ``head, head + 1, ..`` (mod day_cap) of ``day_keys`` i64[day_cap]; -1 for a day the
    ring does not hold.  ts f64[U] on the device."""
    if not isinstance(ts, torch.Tensor) or ts.dtype != torch.float64 or ts.dim() != 1:
        raise ValueError("ts must be a float64 tensor [U]")
    if day_keys.dtype != torch.int64 or day_keys.dim() != 1 or not day_keys.is_contiguous():
        raise ValueError("day_keys must be a contiguous int64 tensor [day_cap]")
    dev = ts.device
    _lib.require_gpu(dev)
    if day_keys.device != dev:
        raise ValueError("all tensors must live on %s" % dev)
    U = int(ts.shape[0])
    slot = torch.empty(U, dtype=torch.int32, device=dev)
    _lib.call("pfo_day_lookup", _lib.ptr(ts.contiguous()), U, day_keys.data_ptr(), int(day_keys.shape[0]), int(head), int(n_days),
              float(key_divisor), slot.data_ptr(), _lib.stream_ptr())
    return slot
