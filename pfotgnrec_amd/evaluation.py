"""``eval_recommendation`` of the reference (evaluation.py:39-264) on the native path.

Per batch: candidate draw, forward-only embeddings of B * (2 + N_ITEMS) roots (``TGN.embed_device``) and ONE launch of
``pfo_eval_metrics`` for everything the reference's per-interaction Python loop computes (ranking, recall / NDCG@{1,3,5}, the
change of annualised return and Sharpe ratio when the top-1/3/5 stocks join the portfolio, in-sample and out-of-sample).
The per-interaction rows stay on the device for the whole pass and are read back once; the 30 averages and ">0" shares are
taken on the host in fp64, over the rows in interaction order, as the reference takes them over its lists.
"""
import math
import os
import pickle

import numpy as np

from . import _lib
from .mv_sampler import day_indices, log_returns, prices_from_time_feature
from .rand_edge_sampler import DeviceNegativeSampler, item_availability, pack_portfolios

TOPK = (1, 3, 5)
ORDER_MODES = {"mv": 0, "basket": 1}     # ``order=`` -> ``mode`` of ``pfo_eval_metrics_mv``; "score" is ``pfo_eval_metrics``


class InvestTables:
    """Past and future prices of every stock per trading day (``time_feature_past_{p}.pkl`` / ``time_feature_future_{p}.pkl``:
    day key -> stock code -> prices) and ``map_item_id`` (stock code -> 0-based item index), as the dense fp64 log-return
    tables ``pfo_eval_metrics`` reads - built exactly as ``MVSampler`` builds its table (``prices_from_time_feature`` +
    ``log_returns``: np.log(p[1:] / p[:-1]) per stock, evaluation.py:31,161,168)."""

    def __init__(self, time_feature_past, time_feature_future, map_item_id, upper_u=None):
        self.map_item_id = map_item_id
        self.upper_u = None if upper_u is None else int(upper_u)
        self.days, past = prices_from_time_feature(time_feature_past, map_item_id, upper_u)
        days_f, future = prices_from_time_feature(time_feature_future, map_item_id, upper_u)
        if [str(d) for d in self.days] != [str(d) for d in days_f]:
            raise ValueError("time_feature_past and time_feature_future list different days")
        self.returns_past, self.returns_future = log_returns(past), log_returns(future)
        self._dev = {}

    @classmethod
    def from_prices(cls, days, prices_past, prices_future, map_item_id, upper_u=None):
        """Dense form: ``days`` the day keys of axis 0, prices f64[day, item, n_prices]; ``upper_u`` is only recorded (``backtest``
        reads it)."""
        self = cls.__new__(cls)
        self.map_item_id, self.days = map_item_id, list(days)
        self.upper_u = None if upper_u is None else int(upper_u)
        self.returns_past, self.returns_future = log_returns(prices_past), log_returns(prices_future)
        if self.returns_past.shape != self.returns_future.shape or len(self.days) != self.returns_past.shape[0]:
            raise ValueError("past / future prices and the day keys differ in shape")
        self._dev = {}
        return self

    @classmethod
    def from_files(cls, period, root="./data", upper_u=None):
        """The three pickles evaluation.py:41-43 opens, under ``{root}/period_{period}/``."""
        d = os.path.join(root, "period_%s" % period)

        def load(name):
            with open(os.path.join(d, name), "rb") as f:
                return pickle.load(f)
        return cls(load("time_feature_past_%s.pkl" % period), load("time_feature_future_%s.pkl" % period),
                   load("map_item_id.pkl"), upper_u)

    @property
    def n_items(self):
        return self.returns_past.shape[1]

    def day_indices(self, timestamps):
        """``str(ts)[:8]`` (evaluation.py:149) -> row of the tables; KeyError for a day the files do not list."""
        return day_indices(timestamps, self.days)

    def device_tables(self, device):
        """(past, future) f64[n_days, n_items, n_ret] on ``device`` (uploaded once per device)."""
        import torch
        device = torch.device(device)
        _lib.require_gpu(device)
        if device not in self._dev:
            self._dev[device] = (torch.from_numpy(self.returns_past).to(device), torch.from_numpy(self.returns_future).to(device))
        return self._dev[device]


def eval_batches(n_instances, batch_size, is_test_run=False):
    """[(s_idx, e_idx)] of the batches evaluation.py:63-74 processes: the last batch is skipped, a test run stops at batch 2."""
    out = []
    for batch in range(math.ceil(n_instances / batch_size)):
        s_idx = batch * batch_size
        e_idx = min(n_instances, s_idx + batch_size)
        if e_idx == n_instances:
            continue
        if is_test_run and batch == 2:
            break
        out.append((s_idx, e_idx))
    return out


def eval_portfolios(portfolios, map_item_id):
    """(port_idx i32[n,W], draw_len i32[n], invest_len i32[n]): the packed stock indices with the '' entries dropped, their
    count as the candidate draw uses it (utils.py:76) and as the investment metrics do: 0 for every row whose list holds a
    '' anywhere - evaluation.py:153 tests ``'' in portfolio``, the whole list counts as empty then."""
    idx, lens = pack_portfolios(portfolios, map_item_id)
    empty = np.fromiter(("" in p for p in portfolios), bool, len(portfolios))
    return idx, lens, np.where(empty, 0, lens).astype(np.int32)


def eval_result_dict(EVAL, rank, invest):
    """The 30-key dict of evaluation.py:209-262 from the per-interaction rows (rank i[n], invest f64[n,12] as
    ``pfo_eval_metrics`` lays it out), in fp64 with np.mean over contiguous columns in interaction order.  Recall and NDCG
    are functions of the integer rank (one test item: hit = rank < k, NDCG = 1 / log2(rank + 2), evaluation.py:11-21) and
    are taken from it in fp64 like the reference's, not from the kernel's fp32 copies."""
    rank = np.asarray(rank, np.int64)
    invest = np.asarray(invest, np.float64)
    n = rank.shape[0]
    if n == 0:
        raise ValueError("no evaluation batch was processed (the last batch is always skipped, evaluation.py:68-69)")
    out = {}
    for name, val in (("recall", lambda k: (rank < k).astype(np.float64)),
                      ("ndcg", lambda k: np.where(rank < k, 1.0 / np.log2(rank + 2.0), 0.0))):
        for k in TOPK:
            out["%s_%s_avg_%d" % (EVAL, name, k)] = np.mean(np.ascontiguousarray(val(k)))
    for t, suffix in ((0, ""), (1, "_")):
        for m, name in ((0, "return"), (1, "sharpe")):
            cols = [np.ascontiguousarray(invest[:, t * 6 + m * 3 + i]) for i in range(3)]
            for k, c in zip(TOPK, cols):
                out["%s_%s_avg_%d%s" % (EVAL, name, k, suffix)] = np.mean(c)
            for k, c in zip(TOPK, cols):
                out["%s_%s_percent_%d%s" % (EVAL, name, k, suffix)] = int((c > 0).sum()) / n
    return out


def _injected(negatives, k, sources, portfolios, n, n_items):
    neg = negatives(k, sources, portfolios) if callable(negatives) else negatives[k]
    neg = np.asarray(neg)
    if neg.shape != (n, n_items):
        raise ValueError("negatives of batch %d have shape %s, expected %s" % (k, neg.shape, (n, n_items)))
    return neg


def check_order(order, mv, upper_u, n_items):
    """The ``order`` / ``mv`` keywords of ``eval_recommendation`` checked on the host (ValueError), before any device work."""
    if not isinstance(order, str) or (order != "score" and order not in ORDER_MODES):
        raise ValueError('order must be "score", "mv" or "basket" (got %r)' % (order,))
    if order == "score":
        return
    if mv is None:
        raise ValueError('order="%s" needs mv (an MVSampler or a PriceLedger): it supplies the return table, gamma and lambda_mv' % order)
    for name in ("returns", "upper_u", "gamma", "lambda_mv", "day_of"):
        if not hasattr(mv, name):
            raise ValueError("mv must carry returns, upper_u, gamma, lambda_mv and day_of (an MVSampler); %s is missing" % name)
    if int(mv.upper_u) != int(upper_u):
        raise ValueError("mv.upper_u is %d, upper_u %d: they number the stocks differently" % (int(mv.upper_u), int(upper_u)))
    if 1 + n_items > _lib.RECOMMEND_MV_MAX_ITEMS:
        raise ValueError('order="%s" ranks at most %d candidates per interaction (N_ITEMS = %d)'
                         % (order, _lib.RECOMMEND_MV_MAX_ITEMS - 1, n_items))


def eval_recommendation_rows(tgn, data, full_data, batch_size, n_neighbors, upper_u, period, is_test_run, *, root="./data",
                             tables=None, map_item_id=None, negatives=None, order="score", mv=None):
    """The pass of ``eval_recommendation``; returns its per-interaction rows as host arrays after ONE read-back:
    dict(rank i32[n], recall f32[n,3], ndcg f32[n,3], top5_pos i32[n,5], top5_item i32[n,5], invest f64[n,12]); under
    ``order="mv"`` / ``"basket"`` also top5_fused f64[n,5] and n_adm i32[n], and rank is ``_lib.EVAL_RANK_NONE`` where the
    positive is not ranked (``eval_metrics_mv``)."""
    import torch
    from .functional import eval_buffers, eval_buffers_mv, eval_metrics, eval_metrics_mv
    from .recommend import mv_device_side
    upper_u = int(upper_u)
    N_ITEMS = len(np.unique(full_data.destinations))                               # evaluation.py:84-85
    check_order(order, mv, upper_u, N_ITEMS)
    _lib.require_gpu(tgn.device)
    if tgn.dp_world != 1:
        raise _lib.PfoError("eval_recommendation runs on one rank (evaluation.py has no data-parallel form)")
    if tables is None:
        tables = InvestTables.from_files(period, root, upper_u)
    if map_item_id is None:
        map_item_id = tables.map_item_id
    dev = tgn.device
    ret_past, ret_future = tables.device_tables(dev)
    batches = eval_batches(len(data.sources), batch_size, is_test_run)
    n_rows = batches[-1][1] if batches else 0
    # whole-pass host work, once: day rows and packed portfolios (no per-interaction work inside the batch loop)
    day = torch.from_numpy(tables.day_indices(data.timestamps[:n_rows])).to(dev)
    p_idx, p_len_draw, p_len_invest = eval_portfolios(data.portfolios[:n_rows], map_item_id)
    port_idx = torch.from_numpy(p_idx).to(dev)
    port_len = torch.from_numpy(p_len_invest).to(dev)
    sampler = None
    if negatives is None:
        n_map = len(map_item_id)
        if upper_u + n_map >= tgn.n_nodes:
            raise IndexError("item node ids reach %d, the model has %d nodes" % (upper_u + n_map, tgn.n_nodes))
        # a fresh seed-2024 stream per batch (evaluation.py:88 -> utils.py:82-84), the set semantics of utils.py:96-111
        sampler = DeviceNegativeSampler(item_availability(full_data.destinations, upper_u, n_map), upper_u, dev, seed=2024)
        port_len_draw = torch.from_numpy(p_len_draw).to(dev)
    served = order != "score"
    if served:
        # the day of every interaction in mv's own numbering, once per pass on the host (a ledger's ordinals become ring slots)
        ret_mv, mv_day = mv_device_side(mv, dev, np.asarray(mv.day_of(data.timestamps[:n_rows])).reshape(-1))
    out = eval_buffers_mv(max(n_rows, 1), dev) if served else eval_buffers(max(n_rows, 1), dev)
    with torch.no_grad():
        tgn.eval()
        for k, (s, e) in enumerate(batches):
            B = e - s
            parts = [(data.timestamps[s:e], np.float64), (tgn._check_nodes(data.sources[s:e], "sources"), np.int32),
                     (tgn._check_nodes(data.destinations[s:e], "destinations"), np.int32),
                     (tgn._check_edges(data.edge_idxs[s:e]), np.int32)]
            if sampler is None:
                neg_host = _injected(negatives, k, data.sources[s:e], data.portfolios[s:e], B, N_ITEMS)
                parts.append((tgn._check_nodes(neg_host, "negatives"), np.int32))
                ts, src, dst, eidx, neg = tgn._batch_to_dev(parts)
            else:
                ts, src, dst, eidx = tgn._batch_to_dev(parts)
                neg = sampler.sample(port_idx[s:e], port_len_draw[s:e], N_ITEMS, 0)
            emb, _ = tgn.embed_device(src, dst, [neg.reshape(-1)], [N_ITEMS], ts, eidx, n_neighbors)
            cand = torch.cat([dst.view(B, 1), neg.view(B, N_ITEMS)], 1)                # evaluation.py:176-178
            if served:
                eval_metrics_mv(emb, B, N_ITEMS, cand, day[s:e], port_idx[s:e], port_len[s:e], ret_past, ret_future, upper_u, ret_mv,
                                mv_day[s:e], float(mv.gamma), float(mv.lambda_mv), ORDER_MODES[order], out=out, out_row0=s)
            else:
                eval_metrics(emb, B, N_ITEMS, cand, day[s:e], port_idx[s:e], port_len[s:e], ret_past, ret_future, upper_u,
                             out=out, out_row0=s)
    names = ("rank", "recall", "ndcg", "top5_pos", "top5_item", "invest", "top5_fused", "n_adm")[:len(out)]
    # one read-back: every buffer's rows as bytes of one device tensor, one copy
    flat = torch.cat([o[:n_rows].reshape(-1).view(torch.uint8) for o in out]).cpu().numpy()
    rows, off = {}, 0
    for name, o in zip(names, out):
        nbytes = o[:n_rows].numel() * o.element_size()
        dt = np.dtype(str(o.dtype).replace("torch.", ""))
        rows[name] = flat[off:off + nbytes].view(dt).reshape((n_rows,) + tuple(o.shape[1:])).copy()
        off += nbytes
    return rows


def eval_recommendation(tgn, data, full_data, batch_size, n_neighbors, upper_u, period, is_test_run, EVAL, *, root="./data",
                        tables=None, map_item_id=None, negatives=None, order="score", mv=None):
    """Drop-in for the reference's ``eval_recommendation`` (evaluation.py:39; the first nine arguments are its own): the
    same 30-key dict ``{EVAL}_recall_avg_1`` ... ``{EVAL}_sharpe_percent_5_``.

    Kept from the reference: eval mode (the model is left in it) and no_grad, the LAST batch is skipped (:68-69),
    ``is_test_run`` stops at batch 2, ``N_ITEMS = len(np.unique(full_data.destinations))`` candidates per interaction drawn
    afresh with seed 2024 every batch, the memory keeps being updated by the positives, day key ``str(ts)[:8]``, a portfolio
    with a '' anywhere counts as empty.

    ``tables``: an ``InvestTables`` (default: read from ``{root}/period_{period}/`` like evaluation.py:41-43);
    ``map_item_id``: default ``tables.map_item_id``.  ``negatives``: None - the candidates are drawn on the device
    (``pfo_neg_draw``: the reference's set semantics, not numpy's MT19937 stream); or a callable
    ``(batch_index, sources, portfolios) -> i64[B, N_ITEMS]``, or a sequence of such arrays indexed by batch: the draw is
    injected (parity runs inject the reference's).
    Ranking ties follow the canonical order (score descending, the larger candidate position first, the
    positive last among its ties) where the reference's ``np.argsort(scores)[::-1]`` is platform-dependent.

    ``order``: which order of an interaction's candidates is evaluated.  "score" (default): the dot-product score alone, the
    reference's - today's path, call for call.  "mv": the order ``TGN.recommend(mv=...)`` serves, the rank fusion of
    main.py:243-289; "basket": the order ``TGN.recommend(mv=..., basket=True)`` serves, re-ranked after each of five picks.  Both
    need ``mv`` - an ``MVSampler``, an object that carries its attributes, or a ``PriceLedger``: it supplies the return table,
    ``gamma`` and ``lambda_mv``, its ``day_of(timestamps)`` the day of every interaction (once per pass, on the host), and its
    ``upper_u`` must be this call's.  The portfolio the order is computed against is the one the investment metrics use, so a
    portfolio with a '' counts as empty on both sides.  A positive that the order does not rank - its stock outside mv's table,
    a constant price series, no day, or under "basket" not among the five picks - is a miss at every k; the same 30 keys.
    Which table ``mv`` was built from is the caller's choice and decides what the out-of-sample columns mean: main.py:88 trains
    with a sampler built from ``time_feature_future``, and an order computed from that table has already seen the window the
    ``_``-suffixed (out-of-sample) keys are measured on - they are then in-sample figures of the ranking, whatever their name.
    Build ``mv`` from ``time_feature_past`` for an out-of-sample reading.
    ValueError before any device work: an unknown ``order``, "mv" / "basket" without ``mv``, ``mv.upper_u != upper_u``, more
    than 2047 candidates (``N_ITEMS``) under "mv" / "basket"."""
    rows = eval_recommendation_rows(tgn, data, full_data, batch_size, n_neighbors, upper_u, period, is_test_run, root=root,
                                    tables=tables, map_item_id=map_item_id, negatives=negatives, order=order, mv=mv)
    return eval_result_dict(EVAL, rows["rank"], rows["invest"])
