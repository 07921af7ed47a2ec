"""The rules of the price ledger in numpy: the ring of days, the shift, carry-forward, growth of both axes, expiry,
persistence and the day lookup.  ``RefLedger`` keeps the ring physically (``ring[slot]``), so slots, ``head`` and the capacity
policy (4 days or ``max(2, max_days)`` at first, doubling when full, a re-layout puts the live days at slot 0) can be compared
with the device ledger's, not only the live-order table."""
import numpy as np


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def close_ok(c):
    return bool(c > 0) and bool(np.isfinite(c))


def keys_of(ts, key_divisor=1e6):
    return np.floor(np.asarray(ts).astype(np.float64) / key_divisor).astype(np.int64)


class RefLedger:
    def __init__(self, n_ret, max_days=None, key_divisor=1e6):
        self.n_ret, self.max_days, self.key_divisor = n_ret, max_days, key_divisor
        self.day_cap = max(2, max_days or 4)
        self.head = self.n_days = self.n_stocks = 0
        self.ring = np.zeros((self.day_cap, 0, n_ret))
        self.ring_keys = np.zeros(self.day_cap, np.int64)
        self.last_close = np.zeros(0)

    @classmethod
    def from_table(cls, keys, returns, last_close, max_days=None, key_divisor=1e6):
        r = cls(returns.shape[2], max_days, key_divisor)
        n = returns.shape[0]
        r.day_cap = max(r.day_cap, n)
        r.ring = np.zeros((r.day_cap,) + returns.shape[1:])
        r.ring[:n] = returns
        r.ring_keys = np.zeros(r.day_cap, np.int64)
        r.ring_keys[:n] = keys
        r.n_days, r.n_stocks, r.last_close = n, returns.shape[1], np.array(last_close, np.float64)
        return r

    def slots(self):
        return [(self.head + i) % self.day_cap for i in range(self.n_days)]

    @property
    def keys(self):
        return self.ring_keys[self.slots()]

    @property
    def table(self):
        """f64[n_days, n_stocks, n_ret] in live order."""
        return self.ring[self.slots()]

    def state(self):
        return dict(day_keys=self.keys.copy(), returns=self.table.copy(), last_close=self.last_close.copy())

    def reserve_days(self, day_cap):
        if day_cap <= self.day_cap:
            return
        live, keys = self.table, self.keys
        self.ring = np.zeros((day_cap,) + self.ring.shape[1:])
        self.ring_keys = np.zeros(day_cap, np.int64)
        self.ring[:self.n_days], self.ring_keys[:self.n_days] = live, keys
        self.day_cap, self.head = day_cap, 0

    def _grow_stocks(self, n):
        if n > self.n_stocks:
            pad = n - self.n_stocks
            self.ring = np.concatenate([self.ring, np.zeros((self.day_cap, pad, self.n_ret))], 1)
            self.last_close = np.concatenate([self.last_close, np.full(pad, np.nan)])
            self.n_stocks = n

    def append_day(self, key, closes, stocks=None, grow=True, newest=None):
        """The kernel's rules: positions with an index outside the table or a close that is not positive and finite are
        skipped, later positions overwrite earlier ones.  ``grow``: host inputs - indices / entries past the live count add
        stocks first; device sparse inputs do not (``grow=False``).  ``newest`` f64[n_stocks]: logarithms to take in place of
        ``np.log``'s where a quotient exists (another faithful libm's - the caller bounds their distance, the reference keeps
        the structure).  Returns the quotients f64[n_stocks], NaN where none."""
        closes = np.asarray(closes, np.float64)
        if stocks is None:
            self._grow_stocks(len(closes))
            stocks = np.arange(len(closes))
        elif grow and len(stocks):
            self._grow_stocks(int(np.max(stocks)) + 1)
        today = np.full(self.n_stocks, np.nan)
        for p in range(len(closes)):                             # sequential: the last valid position wins
            s = int(stocks[p])
            if 0 <= s < self.n_stocks and close_ok(closes[p]):
                today[s] = closes[p]
        if self.n_days == self.day_cap and (self.max_days is None or self.n_days < self.max_days):
            self.reserve_days(2 * self.day_cap)
        prev = self.ring[(self.head + self.n_days - 1) % self.day_cap] if self.n_days else np.zeros((self.n_stocks, self.n_ret))
        if self.max_days is not None and self.n_days == self.max_days:
            self.head, self.n_days = (self.head + 1) % self.day_cap, self.n_days - 1
        new = (self.head + self.n_days) % self.day_cap
        row = np.zeros((self.n_stocks, self.n_ret))
        row[:, :-1] = prev[:, 1:]
        quot = np.full(self.n_stocks, np.nan)
        for s in range(self.n_stocks):
            if not np.isnan(today[s]):
                if not np.isnan(self.last_close[s]):
                    with np.errstate(all="ignore"):
                        quot[s] = today[s] / self.last_close[s]
                        row[s, -1] = np.log(quot[s]) if newest is None else newest[s]
                self.last_close[s] = today[s]
        self.ring[new], self.ring_keys[new] = row, key
        self.n_days += 1
        return quot

    def expire_days(self, before_key):
        n = int(np.sum(self.keys < before_key))
        self.head, self.n_days = (self.head + n) % self.day_cap, self.n_days - n
        return n

    def ordinals(self, ts):
        """Ordinal among the live days per timestamp, -1 for a day that is not held."""
        k, live = keys_of(ts, self.key_divisor), self.keys
        out = np.full(k.shape, -1, np.int32)
        for i, v in enumerate(k.tolist()):
            hit = np.flatnonzero(live == v)
            if hit.size:
                out[i] = hit[0]
        return out

    def lookup(self, ts):
        """Ring slot per timestamp, -1 for a day that is not held."""
        o = self.ordinals(ts)
        return np.where(o >= 0, (o + self.head) % self.day_cap, -1).astype(np.int32)
