"""The holdings ledger behind ``TGN.track_holdings`` / ``update_holdings``: the portfolio each user's newest interaction record
carried, in capacity storage on the model's device.  ``validate`` checks a writer's arguments on the host alone;
the tables are written by ``pfo_holdings_store`` (snapshots) and ``pfo_holdings_apply`` (trades) and read by
``pfo_holdings_gather`` only."""
import collections

import numpy as np
import torch

from . import _lib
from .tables import RowStore

MAX_WIDTH = 256

# a validated write: host arrays (src any integer dtype, idx i32[N, Wp], len i32[N], ts f64[N]) or the same as device tensors
Write = collections.namedtuple("Write", "N on_dev src idx len ts")
# validated trades: host arrays (src / stock / side any integer dtype, ts f64[N], qty f64[N] or None) or the same as device tensors
Trades = collections.namedtuple("Trades", "N on_dev src stock side ts qty")


class Holdings:
    """``idx`` i32[n_nodes, width] stock indices padded with -1, ``len`` i32[n_nodes], ``time`` f64[n_nodes] ("as of"): views of
    the leading ``n_nodes`` rows of storage with ``capacity`` rows; never-written rows and rows behind the live count hold
    (-1, 0, -inf).  The item node of stock ``s`` is ``s + upper_u + 1``.  With ``quantities`` also ``qty`` f64[n_nodes, width],
    the share count of every slot (0.0 at and behind ``len``), in the same storage; None otherwise.  ``counters``: device
    int64[2] - buys that found their row full, sells of a stock the row does not hold - that ``apply`` adds to and no write
    reads back."""

    def __init__(self, n_nodes, capacity, width, upper_u, device, quantities=False):
        self.width, self.upper_u, self.quantities = int(width), int(upper_u), bool(quantities)
        specs = [((self.width,), torch.int32, -1), ((), torch.int32, 0), ((), torch.float64, float("-inf"))]
        if self.quantities:
            specs.append(((self.width,), torch.float64, 0))
        self._store = RowStore.allocate(specs, capacity, n_nodes, torch.device(device))
        self.counters = torch.zeros(2, dtype=torch.int64, device=torch.device(device))
        self._trade_scratch = None
        self._scratch()

    def _scratch(self):
        # scratch of the two native calls, kept between them and re-made with the storage: the store's stamp table, the
        # gather's node id -> position table (neither needs an initial value: include/pfotgn.h)
        self._stamp, self._pos = (torch.empty(self.capacity, dtype=torch.int32, device=self.device) for _ in range(2))

    n_nodes = property(lambda self: self._store.rows)
    capacity = property(lambda self: self._store.capacity)
    device = property(lambda self: self._store.storage[0].device)
    idx = property(lambda self: self._store.views()[0])
    len = property(lambda self: self._store.views()[1])
    time = property(lambda self: self._store.views()[2])
    qty = property(lambda self: self._store.views()[3] if self.quantities else None)

    def resize(self, n_nodes, capacity=None):
        """``n_nodes`` live rows (never fewer than now) in storage of ``capacity`` rows (None: what is there, or just enough):
        live rows keep every bit, new rows hold the initial values."""
        if int(n_nodes) < self.n_nodes:
            raise ValueError("the holdings ledger does not shrink (%d rows live, %d asked for)" % (self.n_nodes, int(n_nodes)))
        if self._store.resize(n_nodes, capacity):
            self._scratch()

    def move(self, device):
        """A device move (``TGN._apply``): the storage travels as a whole, every bit kept (a cast of the model's floating
        tensors does not reach the fp64 times)."""
        self._store.move(lambda t: t.to(device))
        self.counters, self._trade_scratch = self.counters.to(device), None
        self._scratch()

    def store(self, src, port_idx, port_len, ts):
        from .functional import holdings_store
        if self.quantities:
            raise ValueError("a ledger with quantities is written by trades only (trade_holdings): a snapshot carries no share counts")
        holdings_store(src, port_idx, port_len, ts, *self._store.views()[:3], self._stamp)

    def apply(self, src, stock, side, ts, qty=None):
        """Buys and sells of device events (i32 / i32 / i32 / f64 [/ f64]) applied to the rows in event order
        (``pfo_holdings_apply``); the two counters are added to on the device."""
        from .functional import holdings_apply
        need = _lib.byte_count("pfo_holdings_apply_scratch_bytes", max(self.n_nodes, 1), int(src.shape[0]))
        if self._trade_scratch is None or self._trade_scratch.numel() < need:      # (kept between ticks: it follows N alone)
            self._trade_scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
        holdings_apply(src, stock, side, ts, self.idx, self.len, self.time, qty, self.qty, self.counters, self._trade_scratch)

    def gather(self, users, items=None):
        """(port_idx i32[U, width], port_len i32[U], excl_pos i32[U, width] or None without ``items``) for device ``users``."""
        from .functional import holdings_gather
        return holdings_gather(users, self.idx, self.len, self.upper_u, items, self._pos)

    def gather_weights(self, users, mode, last_close=None):
        """The weight rows f64[U, width] of device ``users`` beside ``gather``'s port_idx (``pfo_holdings_gather_weights``):
        ``mode`` "shares" - the share counts - or "value" - share count x ``last_close[stock]`` (f64 [n_stocks] on the device)."""
        from .functional import holdings_gather_weights
        if not self.quantities:
            raise ValueError("weights need a ledger that keeps quantities: track_holdings(width, upper_u, quantities=True)")
        return holdings_gather_weights(users, self.idx, self.len, self.qty, mode, last_close)

    def rows(self, users):
        """``(port_idx i32[U, width], port_len i32[U])`` on the device: the rows of ``users`` (node ids: a host array or an
        integer device tensor); ids outside the table give (-1.., 0)."""
        if not torch.is_tensor(users):
            users = torch.from_numpy(np.ascontiguousarray(np.asarray(users), dtype=np.int32))
        users = users.to(device=self.device, dtype=torch.int32).contiguous()
        return self.gather(users)[:2]


def _fits_i32(a):
    return not a.size or (int(a.min()) >= -(1 << 31) and int(a.max()) < (1 << 31))


def validate(width, n_nodes, sources, portfolios, edge_times):
    """The arguments of a ledger write checked on the host (ValueError) -> ``Write``.  ``portfolios``: a packed pair
    (idx [N, Wp], len [N]) as numpy or as i32 device tensors, or one list of integer stock indices per event.  Host inputs:
    equal lengths, integer dtypes, values that fit int32, len within [0, Wp], no row longer than ``width``, node ids inside
    [0, n_nodes).  Device inputs: shape and dtype only (the kernel's clamping rules apply)."""
    packed = (isinstance(portfolios, (tuple, list)) and len(portfolios) == 2
              and isinstance(portfolios[0], (torch.Tensor, np.ndarray)) and portfolios[0].ndim == 2)
    on_dev = packed and torch.is_tensor(portfolios[0])
    if on_dev != torch.is_tensor(sources) or on_dev != torch.is_tensor(edge_times) or (on_dev and not torch.is_tensor(portfolios[1])):
        raise ValueError("sources, portfolios and edge_times must all be host arrays or all be device tensors")
    if on_dev:
        idx, length = portfolios
        N = int(sources.shape[0]) if sources.dim() == 1 else -1
        if (sources.dtype != torch.int32 or N < 0 or edge_times.dtype != torch.float64 or tuple(edge_times.shape) != (N,)
                or idx.dtype != torch.int32 or idx.shape[0] != N or length.dtype != torch.int32 or tuple(length.shape) != (N,)):
            raise ValueError("device inputs must be i32[N] sources, f64[N] edge_times and an i32 pair (idx [N, Wp], len [N])")
        return Write(N, True, sources, idx, length, edge_times)
    src, ts = np.asarray(sources), np.asarray(edge_times)
    if src.ndim != 1 or ts.ndim != 1 or ts.shape[0] != src.shape[0]:
        raise ValueError("sources, portfolios and edge_times must have the same length")
    N = int(src.shape[0])
    if (N and src.dtype.kind not in "iu") or (N and ts.dtype.kind not in "fiu"):
        raise ValueError("sources must be integers and edge_times numbers")
    if N and (int(src.min()) < 0 or int(src.max()) >= n_nodes):
        raise ValueError("sources holds node ids outside [0, %d)" % n_nodes)
    if packed:
        idx, length = np.asarray(portfolios[0]), np.asarray(portfolios[1])
        if idx.shape[0] != N or tuple(length.shape) != (N,):
            raise ValueError("sources, portfolios and edge_times must have the same length: packed portfolios are (idx [N, Wp], len [N])")
        if (idx.size and idx.dtype.kind not in "iu") or (N and length.dtype.kind not in "iu"):
            raise ValueError("packed portfolios must be integers")
        if not _fits_i32(idx) or not _fits_i32(length):
            raise ValueError("portfolios holds values that do not fit 32 bits")
        if N and (int(length.min()) < 0 or int(length.max()) > idx.shape[1]):
            raise ValueError("portfolio lengths must lie in [0, %d]" % idx.shape[1])
    else:
        try:
            rows = [np.asarray(list(r)).reshape(-1) for r in portfolios]
            if any(r.size and r.dtype.kind not in "iu" for r in rows):
                raise TypeError
        except (TypeError, ValueError):
            raise ValueError("portfolios must be a packed (idx, len) pair or one list of integer stock indices per event") from None
        if len(rows) != N:
            raise ValueError("sources, portfolios and edge_times must have the same length: portfolios lists %d events, sources %d"
                             % (len(rows), N))
        if not all(_fits_i32(r) for r in rows):
            raise ValueError("portfolios holds values that do not fit 32 bits")
        idx = np.full((N, max([r.size for r in rows], default=0)), -1, np.int32)
        length = np.zeros(N, np.int32)
        for e, r in enumerate(rows):
            idx[e, :r.size] = r
            length[e] = r.size
    if N and int(length.max()) > width:
        raise ValueError("a portfolio of %d entries does not fit the ledger's width %d" % (int(length.max()), width))
    return Write(N, False, src, idx.astype(np.int32, copy=False), length.astype(np.int32, copy=False), ts.astype(np.float64, copy=False))


def validate_trades(n_nodes, quantities, sources, stocks, sides, edge_times, qty=None):
    """The arguments of ``trade_holdings`` checked on the host (ValueError) -> ``Trades``.  Host inputs: equal lengths, integer
    dtypes, values that fit int32, node ids inside [0, n_nodes), sides in {-1, +1}, quantities finite and positive when given.
    Device inputs (i32 / i32 / i32 / f64 [/ f64]): shape and dtype only - the kernel's skipping rules apply.  ``quantities``:
    whether the ledger keeps them; ``qty`` on a ledger without them is refused."""
    if qty is not None and not quantities:
        raise ValueError("quantities= needs a ledger that keeps them: track_holdings(width, upper_u, quantities=True)")
    cols = [sources, stocks, sides, edge_times] + ([qty] if qty is not None else [])
    on_dev = torch.is_tensor(sources)
    if any(torch.is_tensor(c) != on_dev for c in cols):
        raise ValueError("sources, stocks, sides, edge_times and quantities must all be host arrays or all be device tensors")
    if on_dev:
        N = int(sources.shape[0]) if sources.dim() == 1 else -1
        want = [torch.int32] * 3 + [torch.float64] * (len(cols) - 3)
        if N < 0 or any(c.dtype != dt or tuple(c.shape) != (N,) for c, dt in zip(cols, want)):
            raise ValueError("device inputs must be i32[N] sources, stocks and sides, f64[N] edge_times and f64[N] quantities")
        return Trades(N, True, sources, stocks, sides, edge_times, qty)
    src, stock, side, ts = (np.asarray(c) for c in cols[:4])
    N = int(src.shape[0]) if src.ndim == 1 else -1
    if N < 0 or any(c.ndim != 1 or c.shape[0] != N for c in (stock, side, ts)):
        raise ValueError("sources, stocks, sides and edge_times must have the same length")
    if N and (any(c.dtype.kind not in "iu" for c in (src, stock, side)) or ts.dtype.kind not in "fiu"):
        raise ValueError("sources, stocks and sides must be integers and edge_times numbers")
    if not all(_fits_i32(c) for c in (src, stock, side)):
        raise ValueError("sources, stocks or sides hold values that do not fit 32 bits")
    if N and (int(src.min()) < 0 or int(src.max()) >= n_nodes):
        raise ValueError("sources holds node ids outside [0, %d)" % n_nodes)
    if N and not np.isin(side, (-1, 1)).all():
        raise ValueError("sides must be +1 (buy) or -1 (sell)")
    if qty is not None:
        qty = np.asarray(qty)
        if qty.ndim != 1 or qty.shape[0] != N:
            raise ValueError("quantities must have the length of sources")
        if N and (qty.dtype.kind not in "fiu" or not (np.isfinite(qty) & (qty > 0)).all()):
            raise ValueError("quantities must be finite and positive")
        qty = qty.astype(np.float64, copy=False)
    return Trades(N, False, src, stock, side, ts.astype(np.float64, copy=False), qty)
