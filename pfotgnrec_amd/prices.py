"""The price ledger: the log-return table of the mean-variance rank, ``returns f64[day, stock, n_ret]``, kept in
capacity storage on the device and advanced in place - one ``append_day`` per trading day (``pfo_returns_append_day``: the
window of day d is the window of day d - 1 shifted by one, so a new day costs one logarithm per stock) - and the trading day
of a timestamp found on the device (``pfo_day_lookup``).  A ``PriceLedger`` is accepted wherever ``TGN.recommend`` takes
``mv=``: it carries ``returns``, ``upper_u``, ``gamma``, ``lambda_mv`` and ``day_of``."""
import bisect
import operator

import numpy as np
import torch

from . import _lib
from .mv_sampler import log_returns

I64_MAX = (1 << 63) - 1


def _key(k, what="day_key"):
    try:
        k = operator.index(k)
    except TypeError:
        raise ValueError("%s must be an integer" % what) from None
    if not -I64_MAX <= k <= I64_MAX:
        raise ValueError("%s does not fit 64 bits" % what)
    return k


class PriceLedger:
    """``returns`` f64[day_cap, stock_cap, n_ret]: the day axis is a RING (``head``, ``n_days`` live slots, live order =
    ``head, head + 1, ..`` mod ``day_cap``), the stock axis holds ``n_stocks`` live rows; rows behind the live count and rows
    never quoted are all zeros - a constant series has y = 0/0, so such a stock is in no order until its window holds two
    different closes.  ``day_keys`` i64[day_cap] strictly increasing in live order (``keys``: the live ones, on the host),
    ``last_close`` f64[n_stocks] NaN until first quoted.  ``max_days=N``: the oldest day leaves when day N + 1 arrives (O(1));
    None: the ring grows geometrically.  The key of a timestamp is ``floor(ts / key_divisor)`` - with 1e6 the ``str(ts)[:8]``
    of a ``yyyymmddHHMMSS`` timestamp.  An explicit day index, and what ``day_of`` returns, is the ORDINAL among the live days
    (0 = oldest); ``slots_of`` turns ordinals into ring slots, which is what the kernels index ``returns`` with.

    A held stock index in [n_stocks, stock_cap) reads a zero row (a stock never quoted), where an ``MVSampler`` ignores an
    index outside its table."""

    def __init__(self, n_ret, upper_u, device, gamma=2.0, lambda_mv=0.5, max_days=None, key_divisor=1e6):
        try:
            n_ret, upper_u = operator.index(n_ret), operator.index(upper_u)
            max_days = None if max_days is None else operator.index(max_days)
        except TypeError:
            raise ValueError("n_ret, upper_u and max_days must be integers") from None
        if not 2 <= n_ret <= 128:
            raise ValueError("n_ret must be in [2, 128] (got %d)" % n_ret)
        if max_days is not None and max_days < 1:
            raise ValueError("max_days must be at least 1")
        key_divisor = float(key_divisor)
        if not (key_divisor > 0 and np.isfinite(key_divisor)):
            raise ValueError("key_divisor must be positive and finite")
        self.n_ret, self.upper_u, self.max_days, self.key_divisor = n_ret, upper_u, max_days, key_divisor
        self.gamma, self.lambda_mv = float(gamma), float(lambda_mv)
        self.head = self.n_days = self.n_stocks = 0
        self.keys = []                                           # the live keys in live order (host mirror of day_keys)
        self._alloc(max(2, max_days or 4), 1, torch.device(device))

    # ------------------------------------------------------------------ storage
    def _alloc(self, day_cap, stock_cap, device):
        self._returns = torch.zeros((day_cap, stock_cap, self.n_ret), dtype=torch.float64, device=device)
        self._day_keys = torch.zeros(day_cap, dtype=torch.int64, device=device)
        self._last_close = torch.full((stock_cap,), float("nan"), dtype=torch.float64, device=device)
        self._stamp = torch.empty(stock_cap, dtype=torch.int32, device=device)     # scratch of the sparse form, any content

    @property
    def device(self):
        return self._returns.device

    @property
    def day_cap(self):
        return int(self._returns.shape[0])

    @property
    def stock_cap(self):
        return int(self._returns.shape[1])

    @property
    def returns(self):
        """The whole storage [day_cap, stock_cap, n_ret]: what the query kernels are given, indexed by ring slot."""
        return self._returns

    @property
    def day_keys(self):
        return self._day_keys

    @property
    def last_close(self):
        return self._last_close[:self.n_stocks]

    def live_slots(self):
        return [(self.head + i) % self.day_cap for i in range(self.n_days)]

    def reserve(self, n_days=None, n_stocks=None):
        """Capacity for ``n_days`` days and ``n_stocks`` stocks (``TGN.reserve``'s contract): live rows keep every bit, capacity
        never shrinks, asking for less than what is live raises ``ValueError``.  A change re-lays the table out (live days in
        order from slot 0) with one strided copy."""
        want = []
        for v, live, cap, what in ((n_days, self.n_days, self.day_cap, "days"), (n_stocks, self.n_stocks, self.stock_cap, "stocks")):
            if v is None:
                want.append(cap)
                continue
            try:
                v = operator.index(v)
            except TypeError:
                raise ValueError("reserve takes integers") from None
            if v < live:
                raise ValueError("the price ledger does not shrink (%d %s live, %d asked for)" % (live, what, v))
            if v >= 1 << 31:
                raise ValueError("%d %s do not fit the tables" % (v, what))
            want.append(max(cap, v))
        if want != [self.day_cap, self.stock_cap]:
            self._relayout(*want)

    def _relayout(self, day_cap, stock_cap):
        old = (self._returns, self._day_keys, self._last_close)
        slots = torch.tensor(self.live_slots(), dtype=torch.int64, device=self.device)
        n, s = self.n_days, self.n_stocks
        self._alloc(day_cap, stock_cap, self.device)
        if n:
            self._returns[:n, :s].copy_(old[0].index_select(0, slots)[:, :s])
            self._day_keys[:n].copy_(old[1].index_select(0, slots))
        self._last_close[:s].copy_(old[2][:s])
        self.head = 0

    # ------------------------------------------------------------------ construction from a price history
    @classmethod
    def from_prices(cls, day_keys, prices, upper_u, device, gamma=2.0, lambda_mv=0.5, max_days=None, key_divisor=1e6):
        """A ledger seeded with ``prices`` f64[day, stock, P] under ``day_keys`` [day] (strictly increasing integers): the table
        is the host ``log_returns(prices)``, bit for bit what ``MVSampler(prices, ...)`` uploads, ``n_ret = P - 1``.
        ``prices[d, i, :]`` are taken to be the closes of stock i UP TO AND INCLUDING day d, so ``last_close`` is
        ``prices[-1, :, -1]`` and the next ``append_day`` continues every window."""
        prices = np.asarray(prices, np.float64)
        if prices.ndim != 3 or prices.shape[2] < 3:
            raise ValueError("prices must be [day, stock, P] with P >= 3")
        ledger = cls(prices.shape[2] - 1, upper_u, device, gamma, lambda_mv, max_days, key_divisor)
        keys = np.asarray(day_keys)
        if keys.ndim != 1 or keys.shape[0] != prices.shape[0]:
            raise ValueError("day_keys must hold one key per day of prices (%d)" % prices.shape[0])
        last = prices[-1, :, -1] if prices.shape[0] else np.full(prices.shape[1], np.nan)
        ledger.load_state(dict(day_keys=keys, returns=log_returns(prices), last_close=last))
        return ledger

    # ------------------------------------------------------------------ persistence
    def state(self):
        """A dict of numpy arrays in live order: ``day_keys`` i64[n_days], ``returns`` f64[n_days, n_stocks, n_ret],
        ``last_close`` f64[n_stocks]; ``load_state`` takes it back bit for bit."""
        slots = torch.tensor(self.live_slots(), dtype=torch.int64, device=self.device)
        ret = self._returns.index_select(0, slots)[:, :self.n_stocks].contiguous()
        return dict(day_keys=np.asarray(self.keys, np.int64), returns=ret.cpu().numpy(), last_close=self.last_close.cpu().numpy().copy())

    def load_state(self, state):
        """Replaces the ledger's content with a ``state()`` dict (checked first, ``ValueError``); capacity is kept or grown."""
        try:
            keys, ret, last = (np.asarray(state[k]) for k in ("day_keys", "returns", "last_close"))
        except (KeyError, TypeError):
            raise ValueError("a ledger state holds day_keys, returns and last_close") from None
        if keys.ndim != 1 or (keys.size and keys.dtype.kind not in "iu"):
            raise ValueError("day_keys must be a 1-D array of integers")
        if ret.ndim != 3 or ret.shape[0] != keys.shape[0] or ret.shape[2] != self.n_ret or tuple(last.shape) != (ret.shape[1],):
            raise ValueError("returns must be [n_days, n_stocks, %d] next to day_keys [n_days] and last_close [n_stocks]" % self.n_ret)
        if ret.dtype != np.float64 or last.dtype != np.float64:
            raise ValueError("returns and last_close must be float64")
        klist = [_key(k, "day_keys") for k in keys.tolist()]
        if any(b <= a for a, b in zip(klist, klist[1:])):
            raise ValueError("day_keys must be strictly increasing")
        n, s = (int(v) for v in ret.shape[:2])
        if self.max_days is not None and n > self.max_days:
            raise ValueError("%d days do not fit max_days = %d" % (n, self.max_days))
        dev = self.device
        self._alloc(max(self.day_cap, n), max(self.stock_cap, s), dev)
        if n:
            self._returns[:n, :s].copy_(torch.from_numpy(np.ascontiguousarray(ret)).to(dev))
            self._day_keys[:n].copy_(torch.from_numpy(np.asarray(klist, np.int64)).to(dev))
        self._last_close[:s].copy_(torch.from_numpy(np.ascontiguousarray(last)).to(dev))
        self.head, self.n_days, self.n_stocks, self.keys = 0, n, s, klist

    # ------------------------------------------------------------------ the daily tick
    def _check_day(self, day_key, closes, stocks):
        """Everything ``append_day`` can refuse, on the host alone -> (key, closes, stocks, on_dev, new live stock count)."""
        key = _key(day_key)
        if self.keys and key <= self.keys[-1]:
            raise ValueError("day_key %d is not above the newest day %d" % (key, self.keys[-1]))
        on_dev = torch.is_tensor(closes)
        if stocks is not None and torch.is_tensor(stocks) != on_dev:
            raise ValueError("closes and stocks must both be host arrays or both be device tensors")
        if on_dev:
            if closes.dtype != torch.float64 or closes.dim() != 1:
                raise ValueError("device closes must be f64[n]")
            n = int(closes.shape[0])
            if stocks is None:
                if n < self.n_stocks:
                    raise ValueError("dense closes hold %d entries, the ledger %d stocks" % (n, self.n_stocks))
                return key, closes, None, True, n
            if stocks.dtype != torch.int32 or tuple(stocks.shape) != (n,):
                raise ValueError("device stocks must be i32[m] next to closes f64[m]")
            return key, closes, stocks, True, self.n_stocks     # (indices are not read back: those outside the table are skipped)
        closes = np.asarray(closes)
        if closes.ndim != 1 or (closes.size and closes.dtype.kind not in "fiu"):
            raise ValueError("closes must be a 1-D array of numbers")
        closes = closes.astype(np.float64)
        quoted = closes if stocks is not None else closes[~np.isnan(closes)]
        if quoted.size and not bool(((quoted > 0) & np.isfinite(quoted)).all()):
            raise ValueError("closes must be positive and finite%s" % ("" if stocks is not None else " (NaN: not quoted today)"))
        if stocks is None:
            if closes.shape[0] < self.n_stocks:
                raise ValueError("dense closes hold %d entries, the ledger %d stocks" % (closes.shape[0], self.n_stocks))
            if closes.shape[0] >= 1 << 31:
                raise ValueError("too many stocks")
            return key, closes, None, False, int(closes.shape[0])
        stocks = np.asarray(stocks)
        if stocks.ndim != 1 or (stocks.size and stocks.dtype.kind not in "iu"):
            raise ValueError("stocks must be a 1-D array of integers")
        if stocks.shape[0] != closes.shape[0]:
            raise ValueError("stocks holds %d entries, closes %d" % (stocks.shape[0], closes.shape[0]))
        if stocks.size:
            if int(stocks.min()) < 0 or int(stocks.max()) >= (1 << 31) - 1:
                raise ValueError("stock indices must lie in [0, 2^31 - 1)")
            if np.unique(stocks).shape[0] != stocks.shape[0]:
                raise ValueError("stocks names a stock twice")
        live = max(self.n_stocks, int(stocks.max()) + 1 if stocks.size else 0)
        return key, closes, stocks.astype(np.int32), False, live

    def append_day(self, day_key, closes, stocks=None):
        """One new trading day under ``day_key`` (above every key held).  Dense: ``closes`` f64[>= n_stocks], NaN = not quoted
        today, entries past the live count add stocks; sparse: ``closes`` f64[m] next to ``stocks`` i32[m].  Host arrays or
        device tensors.  For every live stock the new day's window is the newest day's shifted by one (bitwise) with
        ``log(close / last_close)`` behind it - +0 for a stock not quoted today or never quoted before, whose close is carried
        forward; a new stock's rows of earlier days are zeros; the first day of an empty ledger is all zeros.

        Host inputs are checked before anything is written (``ValueError``): a key not above the newest, closes that are not
        positive and finite, stock indices negative / beyond int32 / repeated, lengths that do not match.  Device inputs are
        checked for shape and dtype only: the kernel skips indices outside the table and closes that are not positive and
        finite; among repeated indices the last valid position wins.  One launch (dense), a memset and two (sparse)."""
        from .functional import returns_append_day, returns_scatter_closes
        key, closes, stocks, on_dev, live = self._check_day(day_key, closes, stocks)
        _lib.require_gpu(self.device)
        if on_dev and (closes.device != self.device or (stocks is not None and stocks.device != self.device)):
            raise ValueError("device inputs must live on %s" % self.device)
        # ---- nothing was written up to here
        if live > self.stock_cap:
            self.reserve(n_stocks=max(live, self.stock_cap + self.stock_cap // 2))
        self.n_stocks = live
        if self.n_days == self.day_cap and (self.max_days is None or self.n_days < self.max_days):
            self.reserve(n_days=2 * self.day_cap)
        # the slot the window is shifted from is taken BEFORE the oldest day leaves: with max_days = 1 they are the same day
        prev = (self.head + self.n_days - 1) % self.day_cap if self.n_days else -1
        if self.max_days is not None and self.n_days == self.max_days:
            self.head, self.n_days = (self.head + 1) % self.day_cap, self.n_days - 1
            del self.keys[0]
        new = (self.head + self.n_days) % self.day_cap              # (day_cap >= 2: never the slot it is shifted from)
        if not on_dev:
            closes = torch.from_numpy(closes).to(self.device)
            stocks = None if stocks is None else torch.from_numpy(stocks).to(self.device)
        stamp = None if stocks is None else returns_scatter_closes(stocks, closes, live, self._stamp)
        returns_append_day(self._returns, self._day_keys, self._last_close, prev, new, live, key, closes, stamp)
        self.n_days += 1
        self.keys.append(key)

    # ------------------------------------------------------------------ retention
    def expire_days(self, before_key):
        """Drops the live days with ``key < before_key`` by moving ``head`` (no data moves); returns how many left."""
        n = bisect.bisect_left(self.keys, _key(before_key, "before_key"))
        self.head, self.n_days = (self.head + n) % self.day_cap, self.n_days - n
        del self.keys[:n]
        return n

    # ------------------------------------------------------------------ the day of a timestamp
    def keys_of(self, timestamps):
        """i64 keys of host timestamps: ``(int64) floor(ts / key_divisor)`` in fp64, the device rule."""
        f = np.floor(np.asarray(timestamps).astype(np.float64) / self.key_divisor)
        if f.size and not bool(((f >= -9.2e18) & (f <= 9.2e18)).all()):
            raise KeyError("a timestamp names no day")
        return f.astype(np.int64)

    def day_of(self, timestamps):
        """Ordinals i32 (0 = oldest live day) of host timestamps; ``KeyError`` for a day the ledger does not hold, like
        ``mv_sampler.day_indices``."""
        k = self.keys_of(timestamps)
        live = np.asarray(self.keys, np.int64)
        pos = np.searchsorted(live, k)
        found = live[np.minimum(pos, live.shape[0] - 1)] == k if live.shape[0] else np.zeros(k.shape, bool)
        if not bool(np.all(found)):
            raise KeyError(int(k[~found].reshape(-1)[0]))
        return pos.astype(np.int32)

    def lookup(self, timestamps):
        """Ring slots i32[U] of DEVICE timestamps f64[U] (``pfo_day_lookup``, no read-back); -1 for a day the ledger does not
        hold - the query kernels give such a user an empty answer."""
        from .functional import day_lookup
        return day_lookup(timestamps, self._day_keys, self.head, self.n_days, self.key_divisor)

    def slots_of(self, ordinals):
        """Ring slots of day ordinals (numpy -> numpy i32, tensor -> tensor i32); -1 for an ordinal outside the live days."""
        if torch.is_tensor(ordinals):
            o = ordinals.to(torch.int64)
            slot = (o + self.head) % self.day_cap
            return torch.where((o >= 0) & (o < self.n_days), slot, torch.full_like(slot, -1)).to(torch.int32)
        o = np.asarray(ordinals).astype(np.int64)
        return np.where((o >= 0) & (o < self.n_days), (o + self.head) % self.day_cap, -1).astype(np.int32)
