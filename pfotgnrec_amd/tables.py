"""Rows with capacity: the one rule of every table that grows.  A ``RowStore`` owns tensors that share a row
capacity and a live row count; the rows behind the live ones hold the tensor's fill value at all times, so a row that comes
alive later starts from the initial state.  Owners keep plain attributes that are ``views()`` and re-make them when the store
changed; nothing outside this file allocates a grown table, slices a store by a live count or works out a capacity."""
import torch


def _grown(capacity, need):
    # geometric growth: a stream of serving ticks reallocates O(log n) times
    return max(int(need), int(capacity) + (int(capacity) >> 1) + 16)


def _filled(shape, fill, **kw):
    return torch.full(shape, fill, **kw) if fill else torch.zeros(shape, **kw)


class RowStore:
    def __init__(self, tensors, fills=None, rows=None):
        """Adopts ``tensors`` as the storage, no copy: all rows live, or the leading ``rows``."""
        self.storage, self.fills = list(tensors), list(fills or [0] * len(tensors))
        self.rows = self.capacity if rows is None else int(rows)

    @classmethod
    def allocate(cls, specs, capacity, rows, device):
        """Fresh storage at the fill values; ``specs``: one (trailing shape, dtype, fill) per tensor."""
        store = cls([torch.empty((0,) + tuple(s), dtype=dt, device=device) for s, dt, _ in specs], [f for _, _, f in specs])
        store.resize(rows, capacity)
        return store

    capacity = property(lambda self: int(self.storage[0].shape[0]))

    def views(self):
        """The live rows: contiguous leading-row views of the storage, same dtypes and trailing shapes."""
        return [t[:self.rows] for t in self.storage]

    def capacity_for(self, rows):
        """What holds ``rows`` rows: the present capacity when it does, the next geometric step otherwise."""
        return self.capacity if int(rows) <= self.capacity else _grown(self.capacity, rows)

    def reserve(self, capacity):
        """Exactly ``capacity`` rows when that is more than there is (never fewer): live rows are copied bit for bit, the rows
        behind them hold the fills.  True when the storage moved."""
        if int(capacity) <= self.capacity:
            return False
        live, self.storage = self.views(), [_filled((int(capacity),) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=t.device)
                                            for t, fill in zip(self.storage, self.fills)]
        for new, old in zip(self.views(), live):
            new.copy_(old)
        return True

    def set_rows(self, rows):
        """``rows`` live rows, never fewer than now, within the capacity: nothing moves."""
        if not self.rows <= int(rows) <= self.capacity:
            raise ValueError("the live rows of a table do not shrink and stay within its capacity (%d rows live, capacity %d, "
                             "%d asked for)" % (self.rows, self.capacity, int(rows)))
        self.rows = int(rows)

    def resize(self, rows, capacity=None):
        """``rows`` live rows in storage of ``capacity`` rows (None: what is there, or just enough).  True when it moved."""
        moved = int(rows) >= self.rows and self.reserve(max(int(rows), int(capacity or 0)))
        self.set_rows(rows)
        return moved

    def trim(self, rows):
        """The one way to FEWER live rows (``TGN.expire``): the caller has put the rows behind ``rows`` back to the fills."""
        if not 0 <= int(rows) <= self.rows:
            raise ValueError("trim to %d rows of %d live ones" % (int(rows), self.rows))
        self.rows = int(rows)

    def move(self, *fns):
        """The whole storage travels through one function per tensor, or one for all (a cast reaches some tensors only)."""
        self.storage = [fn(t).contiguous() for fn, t in zip(fns * len(self.storage) if len(fns) == 1 else fns, self.storage, strict=True)]
