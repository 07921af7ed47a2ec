"""Read-only top-k recommendation behind ``TGN.recommend``: ``validate`` checks the arguments on the host alone (no device is
asked for), ``assemble`` embeds users and candidates on the device and lets ``pfo_recommend_topk`` score and select - or, with
a mean-variance side (``validate_mv``), ``pfo_recommend_mv_topk`` (beyond 2048 candidates ``pfo_recommend_mv_topk_wide``) score,
rank twice, blend and select; with ``basket`` on top
of that, ``pfo_recommend_basket_topk`` re-rank after every pick.  With ``only=`` every user ranks a list of its own:
``pfo_recommend_list_topk`` / ``pfo_recommend_list_mv_topk``.  With ``groups=`` / ``group_cap=`` (``validate_groups``) the three
shared-list launches take their capped entries: at most ``group_cap`` picks of a group in a user's list; with ``held_groups=``
(``validate_held_groups``) their ``_held`` entries: the count of a group starts from what the user holds of it.  With
``portfolio_weights=`` (``validate_weights``) the mean-variance launches take their ``_weighted`` entries: every holding weighs
on y by its size."""
import collections
import operator

import numpy as np
import torch

from . import _lib
from .prices import PriceLedger

Query = collections.namedtuple("Query", "k U I K users users_h items_h timestamps ts_h scalar_ts item_ok ok_h ex_ids ex_len mv held "
                               "only_ids only_len only_held groups group_cap held_mode hg_ids hg_len stock_groups "
                               "weights seen seen_since seen_width seen_max_scan basket",
                               defaults=(None, None, None, None, False, None, None, None, None, None, None, None, None, None, None, 0, False))
# the mean-variance side of a query: the return tables' owner, packed portfolios (host or device), one day index per user
# (with a PriceLedger as the owner: the ORDINAL among its live days, or None - the day is looked up on the device)
MVQuery = collections.namedtuple("MVQuery", "src port_idx port_len day_idx")
HELD = "held"     # ``exclude`` / ``portfolios``: take the rows of the model's holdings ledger (port_idx is None in the MVQuery then)
PORTFOLIOS = "portfolios"   # ``held_groups``: the rows of ``portfolios=``, mapped to groups through ``stock_groups``
SHARES, VALUE = "shares", "value"   # ``portfolio_weights``: the ledger's share counts / share count x the price ledger's last close
SEEN = "seen"     # ``exclude`` / ``only`` / ``portfolios``: what the user's row of the temporal adjacency names before its time


def _is_held(a):
    return isinstance(a, str) and a == HELD


def _is_seen(a):
    return isinstance(a, str) and a == SEEN


def _host(a):
    return None if isinstance(a, torch.Tensor) else np.asarray(a)


def validate_seen(U, any_seen, seen_since=None, seen_width=None, seen_max_scan=0, what="users holds",
                  names=("seen_since", "seen_width", "seen_max_scan")):
    """``seen_since`` / ``seen_width`` / ``seen_max_scan`` of ``TGN.recommend`` and ``backtest`` checked on the host (ValueError)
    -> (since, width, max_scan): since None, a float, or f64 [U] (a host array, or the caller's device tensor as it is).
    ``any_seen``: whether one of ``exclude`` / ``only`` / ``portfolios`` is ``"seen"`` - without it the three are refused.
    ``names``: what the caller calls the three (``TGN.history``: since, width, max_scan) - the messages speak of those."""
    n_since, n_width, n_scan = names
    if not any_seen:
        if seen_since is not None or seen_width is not None or seen_max_scan not in (0, None):
            raise ValueError('seen_since / seen_width / seen_max_scan go with exclude="seen", only="seen" or portfolios="seen"')
        return None, None, 0
    try:
        width = _lib.HISTORY_MAX_WIDTH if seen_width is None else operator.index(seen_width)
        max_scan = 0 if seen_max_scan is None else operator.index(seen_max_scan)
    except TypeError:
        raise ValueError("%s and %s must be integers" % (n_width, n_scan)) from None
    if not 1 <= width <= _lib.HISTORY_MAX_WIDTH:
        raise ValueError("%s must lie in [1, %d] (got %d)" % (n_width, _lib.HISTORY_MAX_WIDTH, width))
    if max_scan < 0:
        raise ValueError("%s must not be negative (got %d)" % (n_scan, max_scan))
    since = seen_since
    if since is not None:
        if not isinstance(since, torch.Tensor):
            try:
                since = np.asarray(since, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError("%s must be a number or hold one per user" % n_since) from None
        elif not since.dtype.is_floating_point:
            since = since.to(torch.float64)
        if since.ndim == 0:
            since = float(since)
        elif tuple(since.shape) != (U,):
            raise ValueError("%s must be a scalar or hold one value per entry: %s %d, got shape %s" % (n_since, what, U, tuple(since.shape)))
    return since, width, max_scan


def _int_vector(a, what, n_nodes):
    h = _host(a)
    t = a if h is None else h
    if t.ndim != 1 or (h is not None and h.size and h.dtype.kind not in "iu") or (
            h is None and (t.dtype.is_floating_point or t.dtype == torch.bool)):
        raise ValueError("%s must be a 1-D array of integer node ids" % what)
    if h is not None and h.size and (int(h.min()) < 0 or int(h.max()) >= n_nodes):
        raise ValueError("%s holds node ids outside [0, %d)" % (what, n_nodes))
    return h


def _is_int_array(t):
    return (t.dtype.kind in "iu") if isinstance(t, np.ndarray) else not (t.dtype.is_floating_point or t.dtype == torch.bool)


def _pack_rows(arg, U, strict, pair_msg, int_msg, names, rows_msg, count_msg, bits_msg):
    """``exclude`` / ``portfolios`` -> (rows i32[U, W] padded with -1, lengths [U]): a packed pair goes through checked (host or
    device), one list per user is packed on the host.  ``strict``: a row of anything but integers is refused, not converted.
    The messages are the caller's (``int_msg`` takes one of ``names``, ``count_msg`` the two user counts)."""
    if (isinstance(arg, (tuple, list)) and len(arg) == 2 and isinstance(arg[0], (torch.Tensor, np.ndarray)) and arg[0].ndim == 2):
        rows, lens = arg
        if not isinstance(lens, (torch.Tensor, np.ndarray)):
            lens = np.asarray(lens)
        if rows.shape[0] != U or tuple(lens.shape) != (U,):
            raise ValueError(pair_msg % U)
        for t, what in zip((rows, lens), names):
            if not _is_int_array(t):
                raise ValueError(int_msg % what)
        return rows, lens
    try:
        lists = [np.asarray(list(r)).reshape(-1) for r in arg]
        if strict and any(r.size and r.dtype.kind not in "iu" for r in lists):
            raise TypeError
        lists = [r.astype(np.int64) for r in lists]
    except (TypeError, ValueError):
        raise ValueError(rows_msg) from None
    if len(lists) != U:
        raise ValueError(count_msg % (len(lists), U))
    rows = np.full((U, max([len(r) for r in lists], default=0)), -1, np.int32)
    lens = np.zeros(U, np.int32)
    for i, r in enumerate(lists):
        if r.size and (int(r.min()) < -(1 << 31) or int(r.max()) >= (1 << 31)):
            raise ValueError(bits_msg)
        rows[i, :len(r)] = r
        lens[i] = len(r)
    return rows, lens


def validate_mv(U, I, mv, portfolios, day_idx, ts_h, scalar_ts, holdings=None, *, max_items=_lib.RECOMMEND_MV_MAX_ITEMS):
    """The mean-variance keywords of ``TGN.recommend`` checked on the host (ValueError) -> ``MVQuery``, or None without any.
    ``max_items``: the bound on I of the kernel the query will take."""
    if _is_held(portfolios) and holdings is None:
        raise ValueError('portfolios="held" needs a holdings ledger: call track_holdings(width, upper_u) first')
    if _is_seen(portfolios) and mv is None:
        raise ValueError('portfolios="seen" needs mv (an MVSampler): its upper_u turns the seen item nodes into stock indices')
    if mv is None:
        if portfolios is not None or day_idx is not None:
            raise ValueError("portfolios / day_idx need mv (an MVSampler): without it the portfolio can only be excluded")
        return None
    for name in ("returns", "upper_u", "gamma", "lambda_mv", "day_of"):
        if not hasattr(mv, name):
            raise ValueError("mv must carry returns, upper_u, gamma, lambda_mv and day_of (an MVSampler); %s is missing" % name)
    if portfolios is None:
        raise ValueError("mv needs portfolios: packed (port_idx [U,W], port_len [U]), one list of stock indices per user, \"held\" or \"seen\"")
    if _is_held(portfolios) and int(mv.upper_u) != holdings.upper_u:
        raise ValueError("mv.upper_u is %d, the holdings ledger's %d: they number the stocks differently" % (int(mv.upper_u), holdings.upper_u))
    if len(mv.returns.shape) != 3:
        raise ValueError("mv.returns must be [n_days, n_stocks, n_ret]")
    if I > max_items:
        raise ValueError("with mv, items may hold at most %d candidates (got %d)" % (max_items, I))
    ledger = isinstance(mv, PriceLedger)
    n_days = mv.n_days if ledger else int(mv.returns.shape[0])   # (a ledger's day_idx counts its LIVE days, 0 = oldest)
    if _is_held(portfolios) or _is_seen(portfolios):
        port_idx = port_len = None
    else:
        port_idx, port_len = _pack_rows(
            portfolios, U, True, "packed portfolios must be (port_idx [U,W], port_len [U]) with U = %d",
            "packed portfolios: %s must be integers", ("port_idx", "port_len"),
            "portfolios must be a packed (port_idx, port_len) pair or one list of integer stock indices per user",
            "portfolios lists %d users, users holds %d", "portfolios holds indices that do not fit 32 bits")
    if day_idx is None:
        if ts_h is None:
            if not ledger:
                raise ValueError("day_idx=None takes the day from mv.day_of(timestamps): that needs timestamps on the host")
            return MVQuery(mv, port_idx, port_len, None)         # device timestamps: one pfo_day_lookup, no read-back
        day = np.asarray(mv.day_of(ts_h.reshape(-1)))
        day = np.broadcast_to(day.reshape(-1), (U,)) if scalar_ts else day
    elif isinstance(day_idx, torch.Tensor):
        day = day_idx
    else:
        day = np.asarray(day_idx)
    if not _is_int_array(day):
        raise ValueError("day_idx must be integers")
    if day.ndim == 0:
        day = day.reshape(1).expand(U) if isinstance(day, torch.Tensor) else np.broadcast_to(day.reshape(1), (U,))
    if tuple(day.shape) != (U,):
        raise ValueError("day_idx must be an integer or hold one value per user (%d), got shape %s" % (U, tuple(day.shape)))
    if isinstance(day, np.ndarray) and day.size and (int(day.min()) < 0 or int(day.max()) >= n_days):
        raise ValueError("day_idx holds days outside [0, %d)" % n_days)
    return MVQuery(mv, port_idx, port_len, day)


def validate_weights(U, portfolio_weights, mv, mvq, portfolios, holdings=None, basket=False, groups=None, what="users holds"):
    """``portfolio_weights`` of ``TGN.recommend`` and ``backtest`` checked on the host (ValueError) -> None without it, ``SHARES``
    / ``VALUE``, or the rows: f64 [U, W] in the shape of the packed portfolios (a host array, or the caller's device tensor as
    it is), lists packed with 0.0 behind each row's length.  ``mvq``: what ``validate_mv`` made of ``portfolios``."""
    if portfolio_weights is None:
        return None
    if mv is None or mvq is None:
        raise ValueError("portfolio_weights needs mv and portfolios: the weights weigh on the mean-variance value alone")
    if basket:
        raise ValueError("portfolio_weights and basket=True cannot be combined: the weight a pick joins the holdings with is undefined")
    if groups is not None:
        raise ValueError("portfolio_weights and groups / group_cap cannot be combined: the capped orders have no weighted form")
    if _is_seen(portfolios):
        raise ValueError('portfolio_weights and portfolios="seen" cannot be combined: the caller cannot align rows it never sees')
    if isinstance(portfolio_weights, str):
        if portfolio_weights not in (SHARES, VALUE):
            raise ValueError('portfolio_weights must be "shares", "value", one list of numbers per user or an f64 [U, W] array')
        if not _is_held(portfolios):
            raise ValueError('portfolio_weights="%s" needs portfolios="held": the weights are the ledger\'s' % portfolio_weights)
        if not holdings.quantities:
            raise ValueError('portfolio_weights="%s" needs a ledger that keeps quantities: track_holdings(width, upper_u, '
                             'quantities=True)' % portfolio_weights)
        if portfolio_weights == VALUE and not isinstance(mv, PriceLedger):
            raise ValueError('portfolio_weights="value" needs mv to be a PriceLedger: the price is its last close')
        return portfolio_weights
    if mvq.port_idx is None:
        raise ValueError('explicit portfolio_weights need explicit portfolios (packed or lists): with portfolios="held" pass "shares" or "value"')
    shape = tuple(mvq.port_idx.shape)
    if isinstance(portfolio_weights, (torch.Tensor, np.ndarray)):
        w = portfolio_weights
        if w.ndim != 2 or tuple(w.shape) != shape:
            raise ValueError("portfolio_weights has shape %s, the packed portfolios %s" % (tuple(w.shape), shape))
        if not (w.dtype.is_floating_point if isinstance(w, torch.Tensor) else w.dtype.kind in "fiu"):
            raise ValueError("portfolio_weights must be numbers")
        return w if isinstance(w, torch.Tensor) else w.astype(np.float64)
    try:
        rows = [np.asarray(list(r), dtype=np.float64).reshape(-1) for r in portfolio_weights]
    except (TypeError, ValueError):
        raise ValueError('portfolio_weights must be "shares", "value", one list of numbers per user or an f64 [U, W] array') from None
    if len(rows) != U:
        raise ValueError("portfolio_weights lists %d users, %s %d" % (len(rows), what, U))
    if isinstance(mvq.port_len, torch.Tensor):
        raise ValueError("portfolio_weights as lists need portfolios on the host: beside device rows pass an f64 [U, W] tensor")
    lens = np.asarray(mvq.port_len).reshape(-1)
    w = np.zeros(shape, np.float64)
    for i, r in enumerate(rows):
        if r.size != int(lens[i]):
            raise ValueError("portfolio_weights lists %d weights for user %d, portfolios %d holdings" % (r.size, i, int(lens[i])))
        w[i, :r.size] = r
    return w


def validate_groups(I, groups, group_cap, only=None, mv=None):
    """``groups`` / ``group_cap`` of ``TGN.recommend`` and ``backtest`` checked on the host (ValueError) -> (groups, group_cap):
    (None, None) without them, else one int32 per candidate (a host array, or the caller's integer device tensor as it is: it
    is not read back) and an int >= 1.  ``only`` / ``mv``: what else the query carries - the cap has no list form and no wide
    mean-variance form."""
    if groups is None and group_cap is None:
        return None, None
    if groups is None or group_cap is None:
        raise ValueError("groups and group_cap go together: one group id per candidate, and how many picks a group may hold")
    try:
        group_cap = operator.index(group_cap)
    except TypeError:
        raise ValueError("group_cap must be an integer") from None
    if group_cap < 1:
        raise ValueError("group_cap must be at least 1 (got %d)" % group_cap)
    try:
        g = groups if isinstance(groups, torch.Tensor) else np.asarray(groups)
    except (TypeError, ValueError):
        raise ValueError("groups must hold one integer per candidate") from None
    if g.ndim != 1 or not _is_int_array(g) and (isinstance(g, torch.Tensor) or g.size):
        raise ValueError("groups must hold one integer per candidate: a 1-D array of integer group ids (negative: no group)")
    if int(g.shape[0]) != I:
        raise ValueError("groups holds %d entries, items %d candidates" % (int(g.shape[0]), I))
    if isinstance(g, np.ndarray):
        if g.size and (int(g.min()) < -(1 << 31) or int(g.max()) >= (1 << 31)):
            raise ValueError("groups holds ids that do not fit 32 bits")
        g = g.astype(np.int32)
    if only is not None:
        raise ValueError("groups and only cannot be combined: the list forms have no capped order")
    if mv is not None and I > _lib.RECOMMEND_MV_MAX_ITEMS:
        raise ValueError("with mv and groups, items may hold at most %d candidates (got %d): the capped order has no wide form"
                         % (_lib.RECOMMEND_MV_MAX_ITEMS, I))
    return g, group_cap


def check_held_width(width):
    """A row of ``held_groups="portfolios"`` is a portfolio row: ``width`` columns must fit the held-group row (ValueError)."""
    if width > _lib.RECOMMEND_HELD_MAX_WIDTH:
        raise ValueError('held_groups="portfolios": rows of up to %d stocks, at most %d' % (width, _lib.RECOMMEND_HELD_MAX_WIDTH))


def validate_held_groups(U, held_groups, stock_groups, groups, holdings=None, portfolios=None, what="users holds"):
    """``held_groups`` / ``stock_groups`` of ``TGN.recommend`` and ``backtest`` checked on the host (ValueError) ->
    (mode, ids, lens, stock_groups): all None without ``held_groups``; mode ``HELD`` / ``PORTFOLIOS`` - the rows are the
    ledger's / the query's portfolios, mapped through ``stock_groups`` (one int32 per stock index, host array or the caller's
    integer device tensor) on the device; mode ``"rows"`` - ids i32[U, W] padded with -1 and lens [U], group ids as given (lists
    packed on the host, a packed pair as it is).  ``U`` rows are expected (``what``: who counts them)."""
    if held_groups is None:
        if stock_groups is not None:
            raise ValueError("stock_groups without held_groups: it maps the stocks of held_groups=\"held\" / \"portfolios\" to groups")
        return None, None, None, None
    if groups is None:
        raise ValueError("held_groups needs groups and group_cap: holdings count against a cap")
    by_stock = isinstance(held_groups, str)
    if by_stock:
        if held_groups not in (HELD, PORTFOLIOS):
            raise ValueError('held_groups must be "held", "portfolios", a list of per-user lists of group ids or a packed (ids, lens) pair')
        if held_groups == HELD and holdings is None:
            raise ValueError('held_groups="held" needs a holdings ledger: call track_holdings(width, upper_u) first')
        if held_groups == PORTFOLIOS and portfolios is None:
            raise ValueError('held_groups="portfolios" needs portfolios (and mv): the rows it maps to groups')
        if stock_groups is None:
            raise ValueError('held_groups="%s" needs stock_groups: one group id per stock index' % held_groups)
        try:
            sg = stock_groups if isinstance(stock_groups, torch.Tensor) else np.asarray(stock_groups)
        except (TypeError, ValueError):
            raise ValueError("stock_groups must hold one integer per stock index") from None
        if sg.ndim != 1 or not _is_int_array(sg) and (isinstance(sg, torch.Tensor) or sg.size):
            raise ValueError("stock_groups must hold one integer per stock index: a 1-D array of integer group ids (negative: no group)")
        if isinstance(sg, np.ndarray):
            if sg.size and (int(sg.min()) < -(1 << 31) or int(sg.max()) >= (1 << 31)):
                raise ValueError("stock_groups holds ids that do not fit 32 bits")
            sg = sg.astype(np.int32)
        return held_groups, None, None, sg
    if stock_groups is not None:
        raise ValueError("stock_groups goes with held_groups=\"held\" / \"portfolios\": explicit rows hold group ids already")
    ids, lens = _pack_rows(
        held_groups, U, True, "packed held_groups must be (ids [U,W], lens [U]) with U = %d", "packed held_groups: %s must be integers",
        ("ids", "lens"), 'held_groups must be "held", "portfolios", a list of per-user lists of integer group ids or a packed (ids, lens) pair',
        "held_groups lists %d users, " + what + " %d", "held_groups holds ids that do not fit 32 bits")
    if ids.shape[1] > _lib.RECOMMEND_HELD_MAX_WIDTH:
        raise ValueError("held_groups lists up to %d ids for a user, at most %d" % (ids.shape[1], _lib.RECOMMEND_HELD_MAX_WIDTH))
    if isinstance(ids, np.ndarray) and ids.size and (int(ids.min()) < -(1 << 31) or int(ids.max()) >= (1 << 31)):
        raise ValueError("held_groups holds ids that do not fit 32 bits")
    return "rows", ids, lens, None


def validate(n_nodes, default_neighbors, users, timestamps, k, items, exclude, item_ok, n_neighbors, mv=None, portfolios=None,
             day_idx=None, holdings=None, basket=False, only=None, *, portfolio_weights=None, groups=None, group_cap=None, held_groups=None,
             stock_groups=None, seen_since=None, seen_width=None, seen_max_scan=0):
    """The arguments of ``TGN.recommend`` checked (ValueError) and brought into one form; what lives in device tensors is
    not read back, except ``items`` once."""
    if only is not None and exclude is not None:
        raise ValueError("only and exclude cannot be combined: list what may be offered, or what may not")
    if only is not None and basket:
        raise ValueError("only and basket=True cannot be combined: the basket has no list form")
    try:
        k = operator.index(k)
    except TypeError:
        raise ValueError("k must be an integer") from None
    if not 1 <= k <= 64:
        raise ValueError("k must be in [1, 64] (got %d)" % k)
    if not isinstance(basket, (bool, np.bool_)):
        raise ValueError("basket must be True or False")
    if basket and mv is None:
        raise ValueError("basket=True needs mv (an MVSampler): a pick changes the order only through the mean-variance rank")
    users_h = _int_vector(users, "users", n_nodes)
    U = int(users.shape[0]) if users_h is None else int(users_h.shape[0])
    items_h = _int_vector(items.detach().cpu().numpy() if isinstance(items, torch.Tensor) else items, "items", n_nodes)
    I = int(items_h.shape[0])
    if I < 1 or I > _lib.RECOMMEND_MAX_ITEMS:
        raise ValueError("items must hold between 1 and %d candidates (got %d)" % (_lib.RECOMMEND_MAX_ITEMS, I))
    if (items_h == 0).any():
        raise ValueError("items holds node 0 (the padding node)")
    if np.unique(items_h).shape[0] != I:
        raise ValueError("items holds duplicates")
    ts_h = _host(timestamps)
    ts_any = timestamps if ts_h is None else ts_h
    scalar_ts = ts_any.ndim == 0
    if not scalar_ts and tuple(ts_any.shape) != (U,):
        raise ValueError("timestamps must be a scalar or hold one value per user (%d), got shape %s" % (U, tuple(ts_any.shape)))
    if ts_h is not None and ts_h.dtype.kind not in "fiu":
        raise ValueError("timestamps must be numbers")
    ok_h = None
    if item_ok is not None:
        ok_any = item_ok if isinstance(item_ok, torch.Tensor) else np.asarray(item_ok)
        if tuple(ok_any.shape) != (I,):
            raise ValueError("item_ok must hold one flag per candidate (%d), got shape %s" % (I, tuple(ok_any.shape)))
        ok_h = _host(item_ok)
    ex_ids = ex_len = None
    if _is_held(exclude):
        if holdings is None:
            raise ValueError('exclude="held" needs a holdings ledger: call track_holdings(width, upper_u) first')
    elif exclude is not None and not _is_seen(exclude):
        ex_ids, ex_len = _pack_rows(
            exclude, U, False, "packed exclude must be (ids [U,W], lens [U]) with U = %d", "packed exclude %s must be integers",
            ("ids", "lens"), "exclude must be None, a list of per-user lists of item ids or a packed (ids, lens) pair",
            "exclude lists %d users, users holds %d", "exclude holds ids that do not fit 32 bits")
    if n_neighbors is None:
        n_neighbors = 20 if default_neighbors is None else default_neighbors
    if basket and I > _lib.RECOMMEND_MV_MAX_ITEMS:
        raise ValueError("with basket=True, items may hold at most %d candidates (got %d): only the plain mean-variance order has "
                         "a form for longer lists" % (_lib.RECOMMEND_MV_MAX_ITEMS, I))
    only_ids = only_len = None
    if _is_held(only):
        if holdings is None:
            raise ValueError('only="held" needs a holdings ledger: call track_holdings(width, upper_u) first')
    elif only is not None and not _is_seen(only):
        only_ids, only_len = _pack_rows(
            only, U, False, "packed only must be (ids [U,W], lens [U]) with U = %d", "packed only %s must be integers",
            ("ids", "lens"), 'only must be None, "held", a list of per-user lists of item ids or a packed (ids, lens) pair',
            "only lists %d users, users holds %d", "only holds ids that do not fit 32 bits")
        if only_ids.shape[1] > _lib.RECOMMEND_LIST_MAX_WIDTH:
            raise ValueError("only lists up to %d ids for a user, at most %d" % (only_ids.shape[1], _lib.RECOMMEND_LIST_MAX_WIDTH))
    seen = (_is_seen(exclude), _is_seen(only), _is_seen(portfolios))
    seen_since, seen_width, seen_max_scan = validate_seen(U, any(seen), seen_since, seen_width, seen_max_scan)
    if seen[2] and mv is None:
        raise ValueError('portfolios="seen" needs mv (an MVSampler): its upper_u turns the seen item nodes into stock indices')
    groups, group_cap = validate_groups(I, groups, group_cap, only, mv)
    hg_ports = None                                                  # held_groups="portfolios" in the score order: the rows serve it alone
    if mv is None and day_idx is None and portfolios is not None and isinstance(held_groups, str) and held_groups == PORTFOLIOS:
        hg_ports, portfolios = portfolios, None
    # (the list form ranks the list alone: with ``only`` the mean-variance order is bound by nothing but the plain bound on I)
    mvq = validate_mv(U, I, mv, portfolios, day_idx, ts_h, scalar_ts, holdings,
                      max_items=_lib.RECOMMEND_MV_MAX_ITEMS if basket else _lib.RECOMMEND_MV_WIDE_MAX_ITEMS)
    held_mode, hg_ids, hg_len, stock_groups = validate_held_groups(U, held_groups, stock_groups, groups, holdings,
                                                                   hg_ports if mvq is None else portfolios)
    if held_mode == PORTFOLIOS and mvq is None:
        if _is_held(hg_ports):                                       # the ledger's rows under their other name
            if holdings is None:
                raise ValueError('portfolios="held" needs a holdings ledger: call track_holdings(width, upper_u) first')
            held_mode = HELD
        else:
            hg_ids, hg_len = _pack_rows(
                hg_ports, U, True, "packed portfolios must be (port_idx [U,W], port_len [U]) with U = %d",
                "packed portfolios: %s must be integers", ("port_idx", "port_len"),
                "portfolios must be a packed (port_idx, port_len) pair or one list of integer stock indices per user",
                "portfolios lists %d users, users holds %d", "portfolios holds indices that do not fit 32 bits")
            check_held_width(hg_ids.shape[1])
    elif held_mode == PORTFOLIOS and mvq.port_idx is not None:
        check_held_width(mvq.port_idx.shape[1])
    weights = validate_weights(U, portfolio_weights, mv, mvq, portfolios, holdings, basket, groups)
    held = (_is_held(exclude), mvq is not None and mvq.port_idx is None and not seen[2])
    return Query(k, U, I, int(n_neighbors), users, users_h, items_h, ts_any, ts_h, scalar_ts, item_ok, ok_h, ex_ids, ex_len, mvq,
                 held if any(held) else None, only_ids, only_len, _is_held(only), groups, group_cap, held_mode, hg_ids, hg_len,
                 stock_groups, weights, seen if any(seen) else None, seen_since, seen_width, seen_max_scan, bool(basket))


def _to_dev(dev, a, dtype):
    if isinstance(a, torch.Tensor):
        return a.to(device=dev, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a).astype(str(dtype).replace("torch.", ""), copy=False)).to(dev)


def mv_device_side(mv, dev, day_idx, user_ts=None):
    """What the kernels read of a mean-variance side ``mv`` (an ``MVSampler``, an object that carries its attributes, or a
    ``PriceLedger``) on ``dev``: (returns f64[n_days, n_stocks, n_ret], day i32[n]).  ``day_idx``: what ``mv.day_of`` returns
    (host array or tensor).  A ledger's kernels index its whole storage - ``day_cap`` x ``stock_cap`` - by ring slot: its day
    ordinals become slots, and with ``day_idx`` None the day is ``pfo_day_lookup`` over ``user_ts`` f64[n] on the device.
    The one place this conversion is written: ``TGN.recommend`` and ``eval_recommendation`` both come here."""
    returns = mv.returns
    if not isinstance(returns, torch.Tensor):
        returns = torch.from_numpy(np.ascontiguousarray(returns, dtype=np.float64))
    returns = returns.to(device=dev, dtype=torch.float64)
    if isinstance(mv, PriceLedger):
        day = mv.lookup(user_ts.contiguous()) if day_idx is None else _to_dev(dev, mv.slots_of(day_idx), torch.int32)
    else:
        day = _to_dev(dev, day_idx, torch.int32)
    return returns, day


def assemble(tgn, q, return_embeddings=False):
    """The device side of ``TGN.recommend`` for a validated query: every (item, distinct timestamp) pair is embedded once (the
    grid of ``TGN._dedup_roots``), users and grid go through ``TGN._embed_readonly``, ``recommend_topk`` scores and selects."""
    from .functional import recommend_list_topk, recommend_topk
    dev, k, U, I = tgn.device, q.k, q.U, q.I

    to_dev = lambda a, dtype: _to_dev(dev, a, dtype)

    with torch.no_grad():
        users_d = to_dev(q.users if q.users_h is None else q.users_h, torch.int32)
        items_d = to_dev(q.items_h, torch.int32)
        user_block = None
        if q.scalar_ts:
            grid_t = to_dev(q.timestamps.reshape(1), torch.float64)
            user_ts = grid_t.expand(U)
        elif q.ts_h is not None:
            uniq, inv = np.unique(q.ts_h.astype(np.float64), return_inverse=True)
            grid_t, user_ts = to_dev(uniq, torch.float64), to_dev(q.ts_h, torch.float64)
            user_block = to_dev(inv.reshape(-1), torch.int32)
        else:
            user_ts = to_dev(q.timestamps, torch.float64)
            grid_t, inv = torch.unique(user_ts, return_inverse=True)
            user_block = inv.to(torch.int32)
        n_t = max(1, int(grid_t.shape[0]))
        if U == 0:
            grid_t, n_t = grid_t[:0], 1
        roots = torch.cat([users_d, items_d.repeat(int(grid_t.shape[0]))]).contiguous()
        root_ts = torch.cat([user_ts, grid_t.repeat_interleave(I)]).contiguous()
        emb = tgn._embed_readonly(roots, root_ts, q.K) if roots.shape[0] else torch.empty((0, tgn.n_node_features), dtype=torch.float32, device=dev)
        user_emb, item_emb = emb[:U], emb[U:]
        if U == 0:
            empty = lambda dt: torch.empty((0, k), dtype=dt, device=dev)
            out = (empty(torch.int32), empty(torch.float32), torch.empty(0, dtype=torch.int32, device=dev))
            if q.mv is not None:
                out += (empty(torch.float64),)
            if return_embeddings:
                out += (user_emb, item_emb, torch.empty(0, dtype=torch.int32, device=dev))
            return out
        excl_pos = excl_len = held_ports = None
        ex_held, port_held = q.held or (False, False)
        group_held = q.held_mode == HELD                               # held_groups="held": the ledger rows, as groups
        h_idx = h_len = None
        if ex_held or port_held or q.only_held or group_held:
            # one gather for whoever asks: the ledger rows of the users, and their stocks as candidate positions
            h_idx, h_len, h_pos = tgn.holdings.gather(users_d, items_d if ex_held or q.only_held else None)
            if ex_held or q.only_held:
                excl_pos, excl_len = h_pos, h_len                     # (with ``only``: the list - see ``listed`` below)
            if port_held:
                held_ports = (h_idx, h_len)
        ex_seen, only_seen, port_seen = q.seen or (False, False, False)
        seen_stock = seen_len = None
        if ex_seen or only_seen or port_seen:
            # one gather over the finder's device CSR for whoever asks: the distinct neighbours before each user's time, as
            # candidate positions (exclude / only) and as stock indices (portfolios)
            want = ("len",) + (("pos",) if ex_seen or only_seen else ()) + (("stock",) if port_seen else ())
            rows = dict(zip(want, seen_rows(tgn, users_d, user_ts, q.seen_since, q.seen_width, q.seen_max_scan, want, items_d,
                                            int(q.mv.src.upper_u) if port_seen else None)))
            seen_len, seen_stock = rows["len"], rows.get("stock")
            if ex_seen or only_seen:
                excl_pos, excl_len = rows["pos"], seen_len            # (with ``only``: the list, newest first)
            if port_seen:
                held_ports = (seen_stock, seen_len)
        listed = q.only_held or q.only_ids is not None or only_seen  # pos / len are the users' own lists, not exclusion lists
        id_rows = (q.only_ids, q.only_len) if q.only_ids is not None else (q.ex_ids, q.ex_len)
        if id_rows[0] is not None and id_rows[0].shape[1] > 0:
            # node id -> position in ``items`` through a table over the node ids (-1: not a candidate)
            pos_of = torch.full((tgn.n_nodes,), -1, dtype=torch.int32, device=dev)
            pos_of[items_d.long()] = torch.arange(I, dtype=torch.int32, device=dev)
            ids = to_dev(id_rows[0], torch.int64)
            inside = (ids >= 0) & (ids < tgn.n_nodes)
            excl_pos = torch.where(inside, pos_of[ids.clamp(0, tgn.n_nodes - 1)], torch.full_like(ids, -1, dtype=torch.int32))
            excl_pos = excl_pos.contiguous()
            excl_len = to_dev(id_rows[1], torch.int32)
        if listed and (excl_pos is None or excl_pos.shape[1] == 0):  # (lists without a column: nobody is offered anything)
            excl_pos = torch.full((U, 1), -1, dtype=torch.int32, device=dev)
            excl_len = torch.zeros(U, dtype=torch.int32, device=dev)
        ok_d = None
        if q.item_ok is not None:
            ok_d = (to_dev(q.item_ok if q.ok_h is None else q.ok_h, torch.int64) != 0).to(torch.uint8)
        cap = {}                                                     # (never with ``only``: validate refuses it)
        if q.groups is not None:
            cap = dict(cand_group=to_dev(q.groups, torch.int32), group_cap=q.group_cap)
        held_rows = ()                                               # (held_group, held_len): per-user rows, they follow the block sort
        if q.held_mode == "rows":
            held_rows = (to_dev(q.hg_ids, torch.int32), to_dev(q.hg_len, torch.int32))
        elif q.held_mode is not None:
            if q.hg_ids is not None:                                 # held_groups="portfolios" in the score order: the rows are the query's own
                s_idx, s_len = to_dev(q.hg_ids, torch.int32), to_dev(q.hg_len, torch.int32)
            elif port_seen and not group_held:                       # held_groups="portfolios" over portfolios="seen"
                s_idx, s_len = seen_stock, seen_len
            elif group_held or q.mv.port_idx is None:                # the ledger's rows (also portfolios="held" asked for as groups)
                s_idx, s_len = h_idx, h_len
            else:
                s_idx, s_len = to_dev(q.mv.port_idx, torch.int32), to_dev(q.mv.port_len, torch.int32)
            held_rows = (stock_rows_to_groups(s_idx, to_dev(q.stock_groups, torch.int32)), s_len)
        if q.mv is not None:
            return _assemble_mv(tgn, q, to_dev, items_d, user_emb, item_emb, user_block, n_t, excl_pos, excl_len, ok_d, return_embeddings,
                                held_ports, user_ts, listed, cap, held_rows, users_d)
        if listed:
            launch = lambda ub, ue, pos, ln: recommend_list_topk(ue, item_emb, k, pos, ln, ub, ok_d, n_blocks=n_t)
        else:
            launch = lambda ub, ue, pos, ln, *held: recommend_topk(ue, item_emb, k, ub, pos, ln, ok_d, n_blocks=n_t, **cap, **_held_kw(held))
        return _select(launch, (user_emb, excl_pos, excl_len) + held_rows, user_block, n_t, items_d, item_emb, return_embeddings,
                       sort=not listed)


def seen_rows(tgn, users_d, ts_d, since, width, max_scan, want, items_d=None, upper_u=None):
    """``history_gather`` over the model's own finder for device ``users_d`` i32[n] at ``ts_d`` f64[n] -> the tensors ``want``
    names.  ``since``: None, a float, or f64 [n] on host or device (``validate_seen``)."""
    from .functional import history_gather
    dev, n = tgn.device, int(users_d.shape[0])
    indptr, nbr, _, adj_ts = tgn.neighbor_finder.device_arrays(dev)
    if since is not None:
        since = torch.full((n,), since, dtype=torch.float64, device=dev) if isinstance(since, float) else _to_dev(dev, since, torch.float64)
    return history_gather(indptr, nbr, adj_ts, users_d, ts_d.contiguous(), width, since, max_scan, items_d, None, upper_u, want)


def stock_rows_to_groups(idx, stock_groups):
    """Rows of stock indices i32[U, W] -> rows of group ids through ``stock_groups`` i32[S], both on the device: an index outside
    [0, S) - the -1 padding too - gives -1, a holding in no group.  No read-back."""
    S = int(stock_groups.shape[0])
    if S == 0 or idx.shape[1] == 0:
        return torch.full_like(idx, -1)
    inside = (idx >= 0) & (idx < S)
    return torch.where(inside, stock_groups[idx.clamp(0, S - 1).long()], torch.full_like(idx, -1)).contiguous()


def _held_kw(held):
    return dict(held_group=held[0], held_len=held[1]) if held else {}


def _select(launch, per_user, user_block, n_t, items_d, item_emb, return_embeddings, sort=True):
    """The tail of ``assemble``: ``launch(user_block, *per_user)`` -> (top_pos, ...) with the users of one block side by side
    (the kernels serve a tile of 16 users in one pass per distinct block), so ``per_user`` - the user embeddings first - follows
    the stable sort by block and the results are put back; positions become item ids.  ``sort`` False: the kernel serves a user
    at a time and takes ``user_block`` as it is (the list forms)."""
    if user_block is not None and n_t > 1 and not sort:
        res = launch(user_block, *per_user)
    elif user_block is not None and n_t > 1:
        order = torch.argsort(user_block, stable=True)
        sel = lambda t: None if t is None else t.index_select(0, order).contiguous()
        res = launch(sel(user_block), *(sel(t) for t in per_user))
        res = tuple(torch.empty_like(t).index_copy_(0, order, t) for t in res)
    else:
        res = launch(None, *per_user)
    top_pos = res[0]
    out = (torch.where(top_pos >= 0, items_d[top_pos.clamp(min=0).long()], torch.full_like(top_pos, -1)),) + res[1:]
    if return_embeddings:
        user_emb = per_user[0]
        if user_block is None:
            user_block = torch.zeros(user_emb.shape[0], dtype=torch.int32, device=user_emb.device)
        out += (user_emb, item_emb, user_block)
    return out


def _assemble_mv(tgn, q, to_dev, items_d, user_emb, item_emb, user_block, n_t, excl_pos, excl_len, ok_d, return_embeddings,
                 held_ports=None, user_ts=None, listed=False, cap=None, held_rows=(), users_d=None):
    """The tail of ``assemble`` under a mean-variance side: ``recommend_mv_topk`` in place of ``recommend_topk``, day and
    portfolio rows following the users through the block sort.  ``held_ports``: the ledger's rows (portfolios="held").
    ``q.basket``: ``recommend_basket_topk`` in its place; more than 2048 candidates: ``recommend_mv_topk_wide``.  With a ``PriceLedger`` the kernels index its storage by ring slot:
    day ordinals become slots, no day index at all is ``pfo_day_lookup`` over ``user_ts`` f64[U] on the device.
    ``listed``: ``excl_pos`` / ``excl_len`` are the users' own lists (``only=``) - ``recommend_list_mv_topk`` whatever I is, no
    workspace and no sort by block.  ``cap``: the cap keywords of the bounded and the basket launch (empty: uncapped; validate
    lets them through with neither ``only`` nor more than 2048 candidates).  ``held_rows``: (held_group, held_len) of the users
    or nothing - they follow the users through the block sort like the portfolio rows.  ``q.weights``: the weight rows
    (``portfolio_weights``) - explicit ones go to the device, ``"shares"`` / ``"value"`` are one ``pfo_holdings_gather_weights``
    over ``users_d``; they follow the users through the block sort like ``port_idx`` and the weighted entries are called."""
    from .functional import recommend_basket_topk, recommend_list_mv_topk, recommend_mv_topk, recommend_mv_topk_wide
    topk = recommend_basket_topk if q.basket else recommend_mv_topk   # (the same arguments and return tuple)
    if q.I > _lib.RECOMMEND_MV_MAX_ITEMS:                             # (never the basket: validate refuses it)
        topk = recommend_mv_topk_wide
    dev, mv = tgn.device, q.mv.src
    returns, day = mv_device_side(mv, dev, q.mv.day_idx, user_ts)
    cand_stock = (items_d - (int(mv.upper_u) + 1)).contiguous()
    if held_ports is not None:
        port_idx, port_len = held_ports
    else:
        port_idx = to_dev(q.mv.port_idx, torch.int32) if q.mv.port_idx.shape[1] > 0 else None
        port_len = to_dev(q.mv.port_len, torch.int32) if port_idx is not None else None
    port_w, weighted = None, q.weights is not None
    if isinstance(q.weights, str):
        port_w = tgn.holdings.gather_weights(users_d, q.weights, mv.last_close if q.weights == VALUE else None)
    elif weighted and port_idx is not None:
        port_w = to_dev(q.weights, torch.float64)

    def launch(ub, ue, pos, ln, day, port_idx, port_len, *held):
        wkw = {}
        if weighted:                                                  # (never with a cap or the basket: validate refuses both)
            held, wkw = (), dict(port_w=held[0])
        if listed:
            top_pos, top_score, top_fused, n_valid = recommend_list_mv_topk(ue, item_emb, q.k, pos, ln, cand_stock, returns, day, port_idx,
                                                                            port_len, float(mv.gamma), float(mv.lambda_mv), ub, ok_d,
                                                                            n_blocks=n_t, **wkw)
        else:
            top_pos, top_score, top_fused, n_valid = topk(ue, item_emb, q.k, cand_stock, returns, day, port_idx, port_len, float(mv.gamma),
                                                          float(mv.lambda_mv), ub, pos, ln, ok_d, n_blocks=n_t, **(cap or {}),
                                                          **_held_kw(held), **wkw)
        return top_pos, top_score, n_valid, top_fused
    per_user = (user_emb, excl_pos, excl_len, day, port_idx, port_len) + ((port_w,) if weighted else tuple(held_rows))
    return _select(launch, per_user, user_block, n_t, items_d, item_emb, return_embeddings, sort=not listed)
