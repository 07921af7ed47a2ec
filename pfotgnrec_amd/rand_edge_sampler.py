"""Candidate-negative draw - host mirror of ``RandEdgeSampler`` (utils/utils.py:65-114) over the
HIP kernel ``pfo_neg_draw``.  Draws are Philox-based: the SET semantics of the reference are kept
(never an item of the user's portfolio, only items seen among the train destinations, without
replacement when enough are available), the MT19937 stream is not.
"""
import numpy as np

from . import _lib

_AVAIL_CACHE = []          # [(dst_list object, checksum, upper_u, n_items, availability)] - at most one entry
_GLOBAL_CALLS = [0]


def _checksum(a):
    """Cheap content fingerprint of an id array: length, ends and a strided sample (an in-place edit of the cached
    array between batches is caught unless it avoids every sampled position)."""
    a = np.asarray(a)
    n = a.shape[0]
    if n == 0:
        return (0,)
    step = max(1, n // 1024)
    return (n, int(a[0]), int(a[-1]), int(np.asarray(a[::step], np.int64).sum()))


def item_availability(dst_list, upper_u, n_items):
    """u8[n_items]: 1 where the item occurs in ``dst_list`` (np.unique(dst_list), utils/utils.py:73)."""
    avail = np.zeros(n_items, np.uint8)
    idx = np.asarray(dst_list, np.int64) - (upper_u + 1)
    idx = idx[(idx >= 0) & (idx < n_items)]
    avail[idx] = 1
    return avail


def pack_portfolios(portfolio_list, map_item_id, width=None):
    """List of stock-code lists -> (i32[B,width] item indices padded with -1, i32[B] lengths); '' dropped (:76).
    One pass over the flattened codes and one scatter (the per-row Python loops of the first version were the largest host
    item of a batch on the drop-in surface: 0.3 ms of a 2.3 ms step at C2, bench.py secondary.drop_in_surface)."""
    n = len(portfolio_list)
    lens_all = np.fromiter((len(sub) for sub in portfolio_list), np.int64, n)
    total = int(lens_all.sum())
    get = map_item_id.__getitem__
    flat = np.fromiter((get(c) if c else -1 for sub in portfolio_list for c in sub), np.int64, total)
    row = np.repeat(np.arange(n), lens_all)
    keep = flat >= 0
    flat, row = flat[keep], row[keep]
    lens = np.bincount(row, minlength=n).astype(np.int32)
    if width is None:
        width = max(1, int(lens.max()) if n else 1)
    out = np.full((n, width), -1, np.int32)
    start = np.cumsum(lens) - lens
    col = np.arange(flat.shape[0]) - np.repeat(start, lens)
    out[row, col] = flat
    return out, lens


_PORT_CACHE = []          # [(base object array, map_item_id, packed idx, packed lens, raw list lengths)] - at most one entry
_PORT_BAD = []            # [(base, map_item_id)] whose whole-array pack failed (a code outside the map somewhere): batches of it
                          # are packed directly, the base is not re-packed per batch
_PORT_MAX_WIDTH = 256     # a base with a longer portfolio is not cached (the packed form is [N, widest] int32)


def _spot_check(a, idx_rows, lens_rows, map_item_id, k=3):
    """A few rows of the batch packed directly against the cached rows: an in-place edit of the dataset that keeps every
    list's length (codes swapped) is caught with probability ~k / rows-changed per batch instead of never."""
    n = a.shape[0]
    for r in {0, n // 2, n - 1} if n >= k else range(n):
        row = [map_item_id[c] for c in a[r] if c]
        if len(row) != int(lens_rows[r]) or any(int(x) != y for x, y in zip(idx_rows[r][:len(row)], row)):
            return False
    return True


def packed_portfolios_of(portfolio_list, map_item_id):
    """``pack_portfolios`` for the way main.py feeds it: ``train_data.portfolios[s_idx:e_idx]`` (main.py:186) is a contiguous
    slice of ONE long-lived object array of stock-code lists, sliced again every batch and every epoch.  That array is packed
    once (vectorised, ~0.6 us per code) and a batch is a slice of the packed form; packing the batch itself was the largest
    host item of the drop-in loop after torch's own (0.3 ms of a 2.3 ms step, bench.py secondary.drop_in_surface).  The
    batch's list lengths are compared with the cached ones (an in-place edit that changes a length drops the cache); anything that is
    not such a slice - small arrays, lists, strided views - is packed directly."""
    a = portfolio_list
    try:
        if not (isinstance(a, np.ndarray) and a.dtype == object and a.ndim == 1 and a.shape[0] > 0):
            return pack_portfolios(a, map_item_id)
        base = a
        while isinstance(base.base, np.ndarray):
            base = base.base
        if not (base.dtype == object and base.ndim == 1 and base.shape[0] >= 4096 and base.flags.c_contiguous and a.strides[0] == base.itemsize):
            return pack_portfolios(a, map_item_id)
        start = (a.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // base.itemsize
        n = a.shape[0]
        if start < 0 or start + n > base.shape[0]:
            return pack_portfolios(a, map_item_id)
        if _PORT_BAD and _PORT_BAD[0][0] is base and _PORT_BAD[0][1] is map_item_id:
            return pack_portfolios(a, map_item_id)
        hit = _PORT_CACHE and _PORT_CACHE[0][0] is base and _PORT_CACHE[0][1] is map_item_id
        if not hit:
            try:
                idx, lens = pack_portfolios(base, map_item_id)
            except Exception:
                _PORT_BAD[:] = [(base, map_item_id)]         # remembered: the fallback stays O(batch)
                return pack_portfolios(a, map_item_id)
            if idx.shape[1] > _PORT_MAX_WIDTH:
                _PORT_BAD[:] = [(base, map_item_id)]
                return pack_portfolios(a, map_item_id)
            _PORT_CACHE[:] = [(base, map_item_id, idx, lens, np.fromiter(map(len, base), np.int64, base.shape[0]))]
        _, _, idx, lens, raw = _PORT_CACHE[0]
        if (not np.array_equal(np.fromiter(map(len, a), np.int64, n), raw[start:start + n])
                or not _spot_check(a, idx[start:start + n], lens[start:start + n], map_item_id)):   # the dataset changed under the cache: repack
            _PORT_CACHE[:] = []
            return pack_portfolios(a, map_item_id)
        return idx[start:start + n], lens[start:start + n]
    except Exception:
        return pack_portfolios(a, map_item_id)


_PORT_DEV = []            # [(packed idx object, device, idx on the device, lens on the device, packed lens object)] - at most one entry
_PORT_DEV_MAX_BYTES = 1 << 30
_AVAIL_DEV = []           # [(availability array object, device, its device copy)] - at most one entry


def _rows_of(rows, base):
    """First row of ``rows`` inside ``base`` when ``rows`` is a run of whole rows of that array (a basic slice of it, same row
    layout, inside its bounds), else None.  Taken from the slice's OWN data pointer: several slices of one packed base may be
    held at once (a train and a validation sampler over one array, a prefetched batch), each names its own rows."""
    if not (isinstance(rows, np.ndarray) and rows.base is base and base.flags.c_contiguous and rows.dtype == base.dtype
            and rows.ndim == base.ndim and rows.shape[1:] == base.shape[1:] and rows.shape[0] > 0
            and rows.strides == base.strides and base.strides[0] > 0):
        return None
    off = rows.__array_interface__["data"][0] - base.__array_interface__["data"][0]
    start, rem = divmod(off, base.strides[0])
    if rem != 0 or start < 0 or start + rows.shape[0] > base.shape[0]:
        return None
    return int(start)


def _device_rows(idx_rows, lens_rows, device):
    """The packed rows of a batch on the device.  A batch that is a slice of the cached packed base (packed_portfolios_of) is a
    slice of ONE device copy of that base, uploaded when the base was packed (<= 1 GiB; a batch costs no host-to-device copy
    then: two pageable copies were ~50 us of a step whose device sits idle meanwhile, bench.py secondary.drop_in_surface);
    anything else is uploaded as it is.  Which rows of the base a batch is comes from the batch's own arrays (_rows_of), never
    from what was packed last."""
    import torch
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:          # ("cuda" and "cuda:0" are ONE cache entry)
        device = torch.device("cuda", torch.cuda.current_device())
    base = idx_rows.base if isinstance(idx_rows, np.ndarray) else None
    if isinstance(base, np.ndarray) and base.ndim == 2:
        hit = _PORT_DEV and _PORT_DEV[0][0] is base and _PORT_DEV[0][1] == device
        if not hit and base.nbytes <= _PORT_DEV_MAX_BYTES and _PORT_CACHE and _PORT_CACHE[0][2] is base:
            lens_base = _PORT_CACHE[0][3]
            _PORT_DEV[:] = [(base, device, torch.from_numpy(base).to(device), torch.from_numpy(lens_base).to(device), lens_base)]
            hit = True
        if hit:
            start, n = _rows_of(idx_rows, base), idx_rows.shape[0]
            if start is not None and _rows_of(lens_rows, _PORT_DEV[0][4]) == start and lens_rows.shape[0] == n:
                return _PORT_DEV[0][2][start:start + n], _PORT_DEV[0][3][start:start + n]
    return (torch.from_numpy(np.ascontiguousarray(idx_rows)).to(device), torch.from_numpy(np.ascontiguousarray(lens_rows)).to(device))


class DeviceNegativeSampler:
    """Device-resident form: availability bitmap uploaded once, portfolios passed as packed tensors."""

    def __init__(self, item_avail, upper_u, device, seed=0):
        import torch
        _lib.require_gpu(device)
        self.device = torch.device(device)
        self.n_items = len(item_avail)
        self.upper_u = int(upper_u)
        self.avail = torch.from_numpy(np.ascontiguousarray(item_avail, np.uint8)).to(self.device)
        self.seed = int(seed)

    def sample(self, port_idx, port_len, size, offset, offset_dev=None):
        """port_idx i32[B,W], port_len i32[B] device tensors -> i32[B,size] item node ids (device).  ``offset_dev``: optional
        1-element int64 device tensor added to ``offset`` on the device (steps captured into a HIP graph)."""
        import torch
        B = port_len.shape[0]
        W = port_idx.shape[1] if port_idx.dim() == 2 else 0
        out = torch.empty((B, size), dtype=torch.int32, device=self.device)
        _lib.call("pfo_neg_draw_dev", _lib.ptr(self.avail), self.n_items, _lib.ptr(port_idx), _lib.ptr(port_len), W, B,
                  size, self.upper_u, self.seed, int(offset), _lib.ptr(offset_dev), _lib.ptr(out), _lib.stream_ptr())
        return out


class RandEdgeSampler:
    """Drop-in for utils/utils.py:65 (constructed per batch by main.py:194,347 / evaluation.py:88)."""

    def __init__(self, src_list, dst_list, portfolio_list, upper_u, map_item_id, seed=None, device=None):
        self.src_list = src_list
        self.upper_u = int(upper_u)
        self.n_items = len(map_item_id)
        # the reference re-runs np.unique(dst_list) every batch (utils.py:73) on the same long-lived array; the bitmap is
        # cached on the array OBJECT (held here, so its id cannot be recycled) plus a content fingerprint
        ck = _checksum(dst_list)
        hit = _AVAIL_CACHE and _AVAIL_CACHE[0][0] is dst_list and _AVAIL_CACHE[0][1:4] == (ck, self.upper_u, self.n_items)
        if not hit:
            _AVAIL_CACHE[:] = [(dst_list, ck, self.upper_u, self.n_items, item_availability(dst_list, self.upper_u, self.n_items))]
        self.item_avail = _AVAIL_CACHE[0][4]
        self.port_idx, self.port_len = packed_portfolios_of(portfolio_list, map_item_id)
        self.seed = seed
        self.device = device

    def sample(self, size):
        import torch
        _lib.require_gpu(self.device)
        device = torch.device("cuda") if self.device is None else torch.device(self.device)
        if self.seed is None:                          # training: a fresh stream every call (utils.py:105,111)
            _GLOBAL_CALLS[0] += 1
            seed, offset = 0x5EED, _GLOBAL_CALLS[0] << 24
        else:                                          # evaluation: same negatives on every run (utils.py:82-84)
            seed, offset = int(self.seed), 0
        if not (_AVAIL_DEV and _AVAIL_DEV[0][0] is self.item_avail and _AVAIL_DEV[0][1] == device):
            _AVAIL_DEV[:] = [(self.item_avail, device, DeviceNegativeSampler(self.item_avail, self.upper_u, device, 0))]
        dev = _AVAIL_DEV[0][2]                         # (the bitmap is cached per dst_list in __init__: one upload per dataset)
        dev.seed = seed
        pi, pl = _device_rows(self.port_idx, self.port_len, device)
        return dev.sample(pi, pl, size, offset).cpu().numpy().astype(np.int64)
