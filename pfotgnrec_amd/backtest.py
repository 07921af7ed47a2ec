"""Backtest of the serving path: a prequential walk over a chronological log - ``TGN.recommend`` for a batch, the
served lists scored against what the users then did (``pfo_list_metrics``), ``TGN.observe`` of the batch - so that every order
``recommend`` serves, at every depth it serves, is held against an outcome.  The per-interaction rows stay on the device for the
whole log and are read back once."""
import operator

import numpy as np
import torch

from . import _lib
from . import recommend as R
from .evaluation import InvestTables
from .prices import PriceLedger


def backtest_result_dict(name, rank, invest, cutoffs):
    """The result dict of ``backtest`` from the per-interaction rows (rank i[n], invest f64[n, 4 n_c] as ``pfo_list_metrics``
    lays it out), in the style of ``eval_result_dict``: ``{name}_recall_avg_{c}``, ``{name}_ndcg_avg_{c}``,
    ``{name}_return_avg_{c}``, ``{name}_return_percent_{c}``, ``{name}_sharpe_avg_{c}``, ``{name}_sharpe_percent_{c}`` and the
    last four again with a trailing ``_`` for the out-of-sample table, for every cutoff c; fp64, np.mean over contiguous columns
    in interaction order.  Recall and NDCG are taken from the integer rank over ALL ``n`` rows.  The investment averages and
    ">0" shares run over the rows whose figures of that table hold no NaN only - ``n_past`` rows in-sample, ``n_future``
    out-of-sample (a row misses a table when its day or one of its stocks lies outside it: a ledger that does not reach
    ``horizon`` days past the interaction yet) - and are NaN when there is no such row.  ``n``, ``n_past`` and ``n_future``
    are keys of the dict."""
    from .functional import check_cutoffs
    rank = np.asarray(rank, np.int64).reshape(-1)
    cuts = check_cutoffs(cutoffs, 64)
    n_c = len(cuts)
    invest = np.asarray(invest, np.float64)
    n = rank.shape[0]
    if invest.shape != (n, 4 * n_c):
        raise ValueError("invest must be [n, 4 * n_cutoffs] = %s, got %s" % ((n, 4 * n_c), invest.shape))
    if n == 0:
        raise ValueError("the log is empty: nothing to average")
    out = {}
    for what, val in (("recall", lambda c: (rank < c).astype(np.float64)),
                      ("ndcg", lambda c: np.where(rank < c, 1.0 / np.log2(rank + 2.0), 0.0))):
        for c in cuts:
            out["%s_%s_avg_%d" % (name, what, c)] = np.mean(np.ascontiguousarray(val(c)))
    counts = []
    for t, suffix in ((0, ""), (1, "_")):
        block = invest[:, t * 2 * n_c:(t + 1) * 2 * n_c]
        ok = ~np.isnan(block).any(axis=1)
        n_ok = int(ok.sum())
        counts.append(n_ok)
        for m, what in ((0, "return"), (1, "sharpe")):
            cols = [np.ascontiguousarray(block[ok, m * n_c + i]) for i in range(n_c)]
            for c, col in zip(cuts, cols):
                out["%s_%s_avg_%d%s" % (name, what, c, suffix)] = np.mean(col) if n_ok else float("nan")
            for c, col in zip(cuts, cols):
                out["%s_%s_percent_%d%s" % (name, what, c, suffix)] = int((col > 0).sum()) / n_ok if n_ok else float("nan")
    out["n"], out["n_past"], out["n_future"] = n, counts[0], counts[1]
    return out


def _length(a):
    return int(a.shape[0]) if hasattr(a, "shape") and len(a.shape) >= 1 else len(a)


def _rows_of_log(arg, N, what):
    """``exclude`` / ``portfolios`` over the whole log -> None, "held", "seen", or a packed pair (rows [N, W], lens [N]) on host or
    device."""
    if arg is None or R._is_held(arg) or R._is_seen(arg):
        return arg
    return R._pack_rows(arg, N, what == "portfolios", "packed " + what + " must be (rows [N,W], lens [N]) with N = %d",
                        "packed " + what + ": %s must be integers", ("rows", "lens"),
                        what + " must be a packed (rows, lens) pair or one list of integers per interaction",
                        what + " lists %d interactions, the log holds %d", what + " holds values that do not fit 32 bits")


def check(tgn, sources, destinations, edge_times, edge_idxs, items, k, cutoffs, batch_size, tables, horizon, mv, basket, exclude,
          portfolios, upper_u, groups=None, group_cap=None, seen_since=None, seen_width=None, seen_max_scan=0, *,
          advance_holdings=False):
    """Everything ``backtest`` refuses on the host, before any device work (ValueError) -> (N, k, cutoffs, batch_size, horizon,
    upper_u, exclude, portfolios, seen), the exclude / portfolios over the whole log as ``_rows_of_log`` leaves them, seen =
    (since, width, max_scan) as ``recommend.validate_seen`` leaves them (since over the whole log).  ``groups`` / ``group_cap``:
    the checks of ``recommend`` (``recommend.validate_groups``), made here once for the whole log.  ``advance_holdings`` needs a
    ledger, whose ``upper_u`` must agree with the others like every known one."""
    from .functional import check_cutoffs
    try:
        k = operator.index(k)
    except TypeError:
        raise ValueError("k must be an integer") from None
    if not 1 <= k <= 64:
        raise ValueError("k must be in [1, 64] (got %d): a list is scored to the depth it is served at" % k)
    cuts = check_cutoffs(cutoffs, k, "k")
    N = _length(sources)
    if any(_length(a) != N for a in (destinations, edge_times, edge_idxs)):
        raise ValueError("sources, destinations, edge_times and edge_idxs must have the same length")
    on_dev = [torch.is_tensor(a) for a in (sources, destinations, edge_times, edge_idxs)]
    if any(on_dev) and not all(on_dev):
        raise ValueError("the log must be all host arrays or all device tensors")
    try:
        batch_size = operator.index(batch_size)
    except TypeError:
        raise ValueError("batch_size must be an integer") from None
    if batch_size < 1:
        raise ValueError("batch_size must be at least 1")
    if isinstance(tables, PriceLedger):
        try:
            horizon = tables.n_ret if horizon is None else operator.index(horizon)
        except TypeError:
            raise ValueError("horizon must be an integer number of trading days") from None
        if horizon < 1:
            raise ValueError("horizon must be at least 1 trading day (got %d)" % horizon)
    elif isinstance(tables, InvestTables):
        if horizon is not None:
            raise ValueError("horizon belongs to a PriceLedger: an InvestTables carries its own future table")
    else:
        raise ValueError("tables must be an InvestTables or a PriceLedger")
    if basket and mv is None:
        raise ValueError("basket=True needs mv")
    R.validate_groups(_length(items), groups, group_cap, None, mv)
    seen = R.validate_seen(N, R._is_seen(exclude) or R._is_seen(portfolios), seen_since, seen_width, seen_max_scan, "the log holds")
    if R._is_seen(portfolios) and mv is None:
        raise ValueError('portfolios="seen" needs mv (an MVSampler): its upper_u turns the seen item nodes into stock indices')
    if mv is not None and portfolios is None:
        raise ValueError("mv needs portfolios: a packed pair over the log, one list of stock indices per interaction, or \"held\"")
    if (R._is_held(exclude) or R._is_held(portfolios)) and tgn.holdings is None:
        raise ValueError('"held" needs a holdings ledger: call track_holdings(width, upper_u) first')
    if advance_holdings and tgn.holdings is None:
        raise ValueError("advance_holdings needs a holdings ledger: call track_holdings(width, upper_u) first")
    known = [(what, int(v)) for what, v in (("upper_u", upper_u), ("tables.upper_u", getattr(tables, "upper_u", None)),
                                            ("mv.upper_u", getattr(mv, "upper_u", None)),
                                            ("the holdings ledger's upper_u", tgn.holdings.upper_u if tgn.holdings is not None else None))
             if v is not None]
    if not known:
        raise ValueError("upper_u is not known: pass upper_u=, or tables / mv that carry it")
    for what, v in known[1:]:
        if v != known[0][1]:
            raise ValueError("%s is %d, %s %d: they number the stocks differently" % (known[0][0], known[0][1], what, v))
    return (N, k, cuts, batch_size, horizon, known[0][1], _rows_of_log(exclude, N, "exclude"), _rows_of_log(portfolios, N, "portfolios"),
            seen)


def check_held_groups(tgn, N, held_groups, stock_groups, groups, pf_log):
    """``held_groups`` / ``stock_groups`` of ``backtest`` over the whole log, checked once and before any device work (ValueError,
    the checks of ``recommend``: ``recommend.validate_held_groups``) -> (mode, rows, stock_groups): mode None without them;
    ``"rows"`` with the packed pair (ids [N, W], lens [N]) on host or device, cut per batch; ``"held"`` / ``"portfolios"`` with
    ``stock_groups`` as one int32 per stock index.  ``pf_log``: the portfolios as ``check`` left them."""
    mode, ids, lens, sg = R.validate_held_groups(N, held_groups, stock_groups, groups, tgn.holdings, pf_log, what="the log holds")
    if mode == R.PORTFOLIOS and not R._is_held(pf_log) and not R._is_seen(pf_log):   # (a ledger row and a seen row fit: 256 at the most)
        R.check_held_width(pf_log[0].shape[1])
    return mode, (ids, lens) if mode == "rows" else None, sg


def check_weights(tgn, N, portfolio_weights, mv, basket, groups, portfolios, pf_log):
    """``portfolio_weights`` of ``backtest`` over the whole log, checked once and before any device work (ValueError, the checks
    of ``recommend``: ``recommend.validate_weights``) -> None, ``"shares"`` / ``"value"``, or f64 rows [N, W] on host or device,
    cut per batch.  ``pf_log``: the portfolios as ``check`` left them."""
    mvq = None
    if mv is not None and pf_log is not None:
        mvq = R.MVQuery(mv, None, None, None) if isinstance(pf_log, str) else R.MVQuery(mv, pf_log[0], pf_log[1], None)
    return R.validate_weights(N, portfolio_weights, mv, mvq, portfolios, tgn.holdings, basket, groups, what="the log holds")


def ledger_days(ledger, timestamps, horizon, device):
    """(past, future) ring slots i32[n] on ``device`` of a ``PriceLedger`` for the interactions' timestamps (host array, or f64
    device tensor: ``lookup``, no read-back): the slot of the interaction's day and of the day ``horizon`` trading days later;
    -1 where the ledger does not hold that day - and for both when it does not hold the interaction's."""
    if torch.is_tensor(timestamps):
        slot = ledger.lookup(timestamps.to(device=device, dtype=torch.float64).contiguous()).to(torch.int64)
        o = torch.where(slot >= 0, (slot - ledger.head) % ledger.day_cap, torch.full_like(slot, -1))
        later = torch.where(o >= 0, o + horizon, torch.full_like(o, -1))
    else:
        key = ledger.keys_of(timestamps).reshape(-1)
        live = np.asarray(ledger.keys, np.int64)
        pos = np.searchsorted(live, key)
        found = live[np.minimum(pos, live.shape[0] - 1)] == key if live.shape[0] else np.zeros(key.shape, bool)
        o = np.where(found, pos, -1).astype(np.int64)
        later = np.where(o >= 0, o + horizon, -1)
    return tuple(R._to_dev(device, ledger.slots_of(d), torch.int32) for d in (o, later))


def _cut(rows, lo, hi):
    return None if rows is None else (rows[0][lo:hi], rows[1][lo:hi])


def _without(ids, truth):
    """The packed id rows with every entry equal to the row's truth set to -1 (``recommend`` ignores those); host or device."""
    if torch.is_tensor(ids):
        t = truth.to(device=ids.device, dtype=ids.dtype).view(-1, 1)
        return torch.where(ids == t, torch.full_like(ids, -1), ids)
    if torch.is_tensor(truth):
        truth = truth.detach().cpu().numpy()
    return np.where(ids == np.asarray(truth).reshape(-1, 1), -1, ids)


def backtest_rows(tgn, sources, destinations, edge_times, edge_idxs, items, k, *, cutoffs=(1, 3, 5), batch_size, tables, horizon=None,
                  mv=None, basket=False, exclude=None, portfolios=None, item_ok=None, n_neighbors=None, keep_truth=True, append=False,
                  upper_u=None, groups=None, group_cap=None, held_groups=None, stock_groups=None, seen_since=None, seen_width=None,
                  seen_max_scan=0, portfolio_weights=None, advance_holdings=False):
    """The walk of ``backtest``; returns its per-interaction rows as host arrays after ONE read-back: dict(rank i32[n],
    recall f32[n, n_c], ndcg f32[n, n_c], invest f64[n, 4 n_c], list_item i32[n, k], n_valid i32[n]) - ``list_item`` the served
    lists, rank ``_lib.EVAL_RANK_NONE`` where the item taken is not in the list."""
    from .functional import list_buffers, list_metrics
    N, k, cuts, batch_size, horizon, upper_u, ex_log, pf_log, (since_log, seen_width, seen_max_scan) = check(
        tgn, sources, destinations, edge_times, edge_idxs, items, k, cutoffs, batch_size, tables, horizon, mv, basket, exclude,
        portfolios, upper_u, groups, group_cap, seen_since, seen_width, seen_max_scan, advance_holdings=bool(advance_holdings))
    hg_mode, hg_log, stock_groups = check_held_groups(tgn, N, held_groups, stock_groups, groups, pf_log)
    w_log = check_weights(tgn, N, portfolio_weights, mv, basket, groups, portfolios, pf_log)
    dev = tgn.device
    _lib.require_gpu(dev)
    if w_log is not None and not isinstance(w_log, str):
        w_log = R._to_dev(dev, w_log, torch.float64)                    # on the device once, cut per batch
    cap = {}
    if groups is not None:
        # on the device once, not once per batch (``recommend`` takes an integer device tensor as it is)
        cap = dict(groups=R._to_dev(dev, groups if torch.is_tensor(groups) else np.asarray(groups), torch.int32), group_cap=group_cap)
    if hg_mode == "rows":
        hg_log = (R._to_dev(dev, hg_log[0], torch.int32), R._to_dev(dev, hg_log[1], torch.int32))
    elif hg_mode is not None:
        cap.update(held_groups=hg_mode, stock_groups=R._to_dev(dev, stock_groups, torch.int32))
    if torch.is_tensor(items):
        items = items.detach().cpu().numpy()                         # (``recommend`` would read it back per query)
    ledger = isinstance(tables, PriceLedger)
    if ledger:
        ret_past = ret_future = tables.returns
        day_past, day_future = ledger_days(tables, edge_times, horizon, dev)
    else:
        ret_past, ret_future = tables.device_tables(dev)
        ts_h = edge_times.detach().cpu().numpy() if torch.is_tensor(edge_times) else np.asarray(edge_times)
        day_past = day_future = R._to_dev(dev, np.asarray(tables.day_indices(ts_h)).reshape(-1), torch.int32)
    truth = R._to_dev(dev, destinations, torch.int32)
    users_d = R._to_dev(dev, sources, torch.int32)
    held_ex, held_pf = R._is_held(ex_log), R._is_held(pf_log)
    if advance_holdings:                                              # the batch's interactions as buys, all on the device once
        buy_stock, buy_side = truth - (upper_u + 1), torch.ones_like(users_d)
        buy_ts = R._to_dev(dev, edge_times, torch.float64)
    seen_ex, seen_pf = R._is_seen(ex_log), R._is_seen(pf_log)
    if seen_ex or seen_pf:
        times_d = R._to_dev(dev, edge_times, torch.float64)
        if since_log is not None and not isinstance(since_log, float):
            since_log = R._to_dev(dev, since_log, torch.float64)       # on the device once, cut per batch
    pf_dev = None
    if pf_log is not None and not held_pf and not seen_pf and pf_log[0].shape[1] > 0:
        pf_dev = (R._to_dev(dev, pf_log[0], torch.int32), R._to_dev(dev, pf_log[1], torch.int32))
    n_c = len(cuts)
    out = list_buffers(max(N, 1), n_c, dev)
    lists = torch.empty((max(N, 1), k), dtype=torch.int32, device=dev)
    n_valid_all = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
    for lo in range(0, N, batch_size):
        hi = min(N, lo + batch_size)
        held_rows = tgn.holdings.rows(users_d[lo:hi]) if (held_pf or (held_ex and keep_truth)) else None
        ex = ex_log
        seen_pair = None
        if seen_ex or seen_pf:
            # ONE gather a batch for whoever asks - the query and the metrics: ``recommend`` gets the rows as packed device pairs
            # (item nodes to exclude, the truth taken out on the device with ``keep_truth``; stock indices as the portfolio)
            since = since_log if since_log is None or isinstance(since_log, float) else since_log[lo:hi]
            want = ("len",) + (("node",) if seen_ex else ()) + (("stock",) if seen_pf else ())
            seen_rows = dict(zip(want, R.seen_rows(tgn, users_d[lo:hi], times_d[lo:hi], since, seen_width, seen_max_scan, want,
                                                   None, upper_u if seen_pf else None)))
            if seen_ex:
                ex = (_without(seen_rows["node"], truth[lo:hi]) if keep_truth else seen_rows["node"], seen_rows["len"])
            if seen_pf:
                seen_pair = (seen_rows["stock"], seen_rows["len"])
        if held_ex and keep_truth:
            # the ledger's rows as item ids, the truth taken out on the device: what exclude="held" excludes, minus that item
            h_idx, h_len = held_rows
            ids = torch.where(h_idx >= 0, h_idx + (tgn.holdings.upper_u + 1), torch.full_like(h_idx, -1))
            ex = (_without(ids, truth[lo:hi]), h_len)
        elif ex_log is not None and not held_ex and not seen_ex:
            ex = _cut(ex_log, lo, hi)
            if keep_truth:
                ex = (_without(ex[0], truth[lo:hi] if torch.is_tensor(ex[0]) else destinations[lo:hi]), ex[1])
        mv_side = {}
        if mv is not None:
            mv_side = dict(mv=mv, portfolios=seen_pair if seen_pf else pf_log if held_pf else _cut(pf_log, lo, hi), basket=bool(basket))
            if w_log is not None:
                mv_side["portfolio_weights"] = w_log if isinstance(w_log, str) else w_log[lo:hi]
        if hg_mode == "rows":
            cap["held_groups"] = _cut(hg_log, lo, hi)
        elif hg_mode == R.PORTFOLIOS and mv is None:                  # (the score order: the rows go along for the groups alone)
            cap["portfolios"] = pf_log if held_pf else _cut(pf_log, lo, hi)     # (never "seen": that needs mv)
        res = tgn.recommend(sources[lo:hi], edge_times[lo:hi], k, items, exclude=ex, item_ok=item_ok, n_neighbors=n_neighbors, **mv_side, **cap)
        item_ids, n_valid = res[0], res[2]
        if seen_pf:
            pidx, plen = seen_pair
        else:
            pidx, plen = held_rows if held_pf else (_cut(pf_dev, lo, hi) if pf_dev is not None else (None, None))
        list_metrics(item_ids, truth[lo:hi], cuts, pidx, plen, upper_u, ret_past, day_past[lo:hi], ret_future, day_future[lo:hi],
                     n_valid, out=out, out_row0=lo)
        lists[lo:hi].copy_(item_ids)
        n_valid_all[lo:hi].copy_(n_valid)
        tgn.observe(sources[lo:hi], destinations[lo:hi], edge_times[lo:hi], edge_idxs[lo:hi], batch_size=None, append=append)
        if advance_holdings:
            tgn.holdings.apply(users_d[lo:hi], buy_stock[lo:hi], buy_side[lo:hi], buy_ts[lo:hi])
    names = ("rank", "recall", "ndcg", "invest", "list_item", "n_valid")
    bufs = out + (lists, n_valid_all)
    # one read-back: every buffer's rows as bytes of one device tensor, one copy
    flat = torch.cat([o[:N].reshape(-1).view(torch.uint8) for o in bufs]).cpu().numpy()
    rows, off = {}, 0
    for name, o in zip(names, bufs):
        nbytes = o[:N].numel() * o.element_size()
        dt = np.dtype(str(o.dtype).replace("torch.", ""))
        rows[name] = flat[off:off + nbytes].view(dt).reshape((N,) + tuple(o.shape[1:])).copy()
        off += nbytes
    return rows


def backtest(tgn, sources, destinations, edge_times, edge_idxs, items, k, *, cutoffs=(1, 3, 5), batch_size, tables, horizon=None,
             mv=None, basket=False, exclude=None, portfolios=None, item_ok=None, n_neighbors=None, keep_truth=True, append=False,
             name="backtest", upper_u=None, groups=None, group_cap=None, held_groups=None, stock_groups=None, seen_since=None,
             seen_width=None, seen_max_scan=0, portfolio_weights=None, advance_holdings=False):
    """The served lists of a model held against what happened: a prequential walk over a chronological log (numpy arrays like
    the entry points, or device tensors i32 / i32 / f64 / i32).  Per batch ``[lo, hi)`` of ``batch_size`` interactions:

    1. ``tgn.recommend(sources[lo:hi], edge_times[lo:hi], k, items, ...)`` - ``exclude``, ``item_ok``, ``n_neighbors``, ``mv``,
       ``portfolios``, ``basket``, ``groups`` and ``group_cap`` are passed through, so every served order, the wide mean-variance form, ``"held"`` and a
       ``PriceLedger`` as ``mv`` work as they do there.  ``exclude`` / ``portfolios`` cover the whole LOG here: a packed pair
       (rows [N, W], lens [N]) on host or device, one list per interaction, ``"held"``, or ``"seen"``: what the user's row of the
       finder names strictly before the interaction's time (``seen_since`` - a scalar or one value per interaction -,
       ``seen_width`` and ``seen_max_scan`` as in ``recommend``).  The comparison being strict, a finder built over the FULL log
       serves the walk without ``append``: at every step a user has seen exactly its earlier interactions.
    2. ``list_metrics`` of the lists against ``destinations[lo:hi]`` - the place of the item the user took, and what the first
       c stocks of the list would have done to the portfolio (``portfolios``; None: empty) for every c of ``cutoffs`` (each in
       [1, k]) - written into one set of device buffers for the whole log.
    3. ``tgn.observe`` of the batch (``batch_size=None``, ``append``): the model's state advances exactly as ``observe`` over
       the log with this ``batch_size`` would advance it.  The holdings ledger is not written - unless
       ``advance_holdings=True`` (needs a ledger): then
    4. the batch's interactions are applied to the ledger as buys of stock ``destination - upper_u - 1`` by their sources
       (``pfo_holdings_apply``; quantity 1.0 on a ledger with quantities), so that ``"held"`` is what the user held before THAT
       batch, not before the log.  No sells: a walk observes interactions only.

    One read-back at the end.  The LAST batch is not skipped and there is no ``is_test_run``: this is not the reference's
    evaluation protocol (``eval_recommendation`` is) and shares none of its limits - any k up to 64, up to 65536 candidates.

    ``tables``: where the returns that then happened are read.  An ``InvestTables``: its past / future tables at
    ``tables.day_indices(edge_times)`` (KeyError for a day it does not list).  Or a ``PriceLedger``: in-sample = the window of
    the interaction's day, out-of-sample = the window of the day ``horizon`` trading days later (default ``n_ret``: exactly
    the ``n_ret`` returns that follow), both read from the ledger's own storage by ring slot; where the ledger does not hold
    that day (yet) the row counts in ``n`` but not in ``n_future`` / ``n_past``.  ``upper_u`` (a stock's item node is stock +
    upper_u + 1) is taken from ``tables``, ``mv`` or the holdings ledger, or passed; they must agree.

    ``keep_truth=True``: the item the user is about to take is removed from the user's exclusion row before the query (entries
    set to -1, on the device for ``"held"``, ``"seen"`` and packed device rows), so it is always admissible - as the positive is in the
    reference's protocol; ``False`` leaves the rows alone, and a user who re-buys a held stock can only be missed.

    Returns a dict in the style of ``eval_result_dict`` (``backtest_result_dict``): ``{name}_recall_avg_{c}``,
    ``{name}_ndcg_avg_{c}`` over all ``n`` rows in fp64 from the integer rank; ``{name}_return_avg_{c}``,
    ``{name}_return_percent_{c}``, ``{name}_sharpe_avg_{c}``, ``{name}_sharpe_percent_{c}`` in-sample and the same with a
    trailing ``_`` out-of-sample; and ``n``, ``n_past``, ``n_future``.  The investment averages and ">0" shares run over the
    rows whose figures of that table hold no NaN only (``n_past`` / ``n_future`` of them), not over ``n``.
    ``backtest_rows`` returns the per-interaction rows instead.

    ValueError before any device work: cutoffs not strictly increasing or outside [1, k], k > 64, arrays of unequal length,
    batch_size < 1, ``tables`` of neither kind, a ledger with horizon < 1, ``mv.upper_u`` different from ``tables``', and what
    ``recommend`` refuses of ``groups`` / ``group_cap`` (one without the other, a wrong length, non-integers, a cap below 1,
    with ``mv`` more than 2048 candidates) and of ``held_groups`` / ``stock_groups`` - forwarded too, ``held_groups`` over the whole
    LOG like ``exclude``: a packed pair (ids [N, W], lens [N]), one list of group ids per interaction, ``"held"`` or
    ``"portfolios"`` (without ``groups``, ``"held"`` without a ledger or ``stock_groups``, rows longer than 256, non-integers).

    ``portfolio_weights`` (by name) is forwarded as well, over the whole LOG like ``portfolios``: one list of numbers per
    interaction, an f64 [N, W] array or tensor in the shape of the packed portfolios, or ``"shares"`` / ``"value"`` beside
    ``portfolios="held"`` - and what ``recommend`` refuses of it is refused here, before any device work.  With
    ``advance_holdings=True`` the buys the walk applies carry one share each, as without weights."""
    rows = backtest_rows(tgn, sources, destinations, edge_times, edge_idxs, items, k, cutoffs=cutoffs, batch_size=batch_size,
                         tables=tables, horizon=horizon, mv=mv, basket=basket, exclude=exclude, portfolios=portfolios, item_ok=item_ok,
                         n_neighbors=n_neighbors, keep_truth=keep_truth, append=append, upper_u=upper_u, groups=groups, group_cap=group_cap,
                         held_groups=held_groups, stock_groups=stock_groups, seen_since=seen_since, seen_width=seen_width,
                         seen_max_scan=seen_max_scan, advance_holdings=advance_holdings, portfolio_weights=portfolio_weights)
    return backtest_result_dict(name, rows["rank"], rows["invest"], cutoffs)
