"""The holdings ledger behind ``TGN.track_holdings`` / ``update_holdings``: the portfolio each user's newest interaction record
carried, in capacity storage on the model's device.  ``validate`` checks a writer's arguments on the host alone;
the tables are written by ``pfo_holdings_store`` and read by ``pfo_holdings_gather`` only."""
import collections

import numpy as np
import torch

from .tables import RowStore

MAX_WIDTH = 256

# a validated write: host arrays (src any integer dtype, idx i32[N, Wp], len i32[N], ts f64[N]) or the same as device tensors
Write = collections.namedtuple("Write", "N on_dev src idx len ts")


class Holdings:
    """``idx`` i32[n_nodes, width] stock indices padded with -1, ``len`` i32[n_nodes], ``time`` f64[n_nodes] ("as of"): views of
    the leading ``n_nodes`` rows of storage with ``capacity`` rows; never-written rows and rows behind the live count hold
    (-1, 0, -inf).  The item node of stock ``s`` is ``s + upper_u + 1``."""

    def __init__(self, n_nodes, capacity, width, upper_u, device):
        self.width, self.upper_u = int(width), int(upper_u)
        specs = [((self.width,), torch.int32, -1), ((), torch.int32, 0), ((), torch.float64, float("-inf"))]
        self._store = RowStore.allocate(specs, capacity, n_nodes, torch.device(device))
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
        self._scratch()

    def store(self, src, port_idx, port_len, ts):
        from .functional import holdings_store
        holdings_store(src, port_idx, port_len, ts, *self._store.views(), self._stamp)

    def gather(self, users, items=None):
        """(port_idx i32[U, width], port_len i32[U], excl_pos i32[U, width] or None without ``items``) for device ``users``."""
        from .functional import holdings_gather
        return holdings_gather(users, self.idx, self.len, self.upper_u, items, self._pos)

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
