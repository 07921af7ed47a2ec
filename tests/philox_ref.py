"""Host model of the library's random streams: Philox4x32-10 and the three consumers that turn its words into decisions
(uniform neighbour positions, the candidate / negative draw, the attention dropout keep bits).  Numpy only, no import of the
package: written from the kernel text (csrc/common.hpp ``pfo_philox``, csrc/sampler.hip, csrc/attn_dev.hpp ``attn_keep_bits``),
vectorised in uint64.  All three consumers are pure functions of integers, so the kernels are held to this bit for bit.

| consumer                 | counter (lo, hi)              | word -> decision                                                    |
| uniform positions        | (q, offset + (j >> 2))        | idx = (word[j & 3] * cnt) >> 32, clamped to [0, cnt)                 |
| candidate draw           | (b + offset, k >> 2)          | partial Fisher-Yates when n_avail >= size, else list[(word * n) >> 32] |
| dropout keep, head h     | (n * 64 + lane, offset)       | word[h] >= uint32(min(p * 2^32, 4294967040)), threshold in fp32      |
"""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)       # round multipliers
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)       # key increments (golden ratio, sqrt(3) - 1)
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _u64(x):
    """Any integer in [0, 2^64) (Python int, numpy integer or array) as a uint64 array."""
    if isinstance(x, np.ndarray):
        if x.dtype == np.uint64:
            return x
        assert x.dtype.kind in "iu" and (x.size == 0 or x.min() >= 0), "counters are unsigned"
        return x.astype(np.uint64)
    return np.asarray(int(x) & 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)


def philox4x32_10(seed, ctr_lo, ctr_hi):
    """uint32[..., 4]: key = (seed low, seed high), counter = (lo low, lo high, hi low, hi high), ten rounds.  The arguments
    broadcast against each other; every 32-bit quantity is carried in a uint64 (32 x 32 -> 64 bit products never wrap)."""
    seed, lo, hi = np.broadcast_arrays(_u64(seed), _u64(ctr_lo), _u64(ctr_hi))
    k0, k1 = seed & _LO, seed >> _S32
    c0, c1, c2, c3 = lo & _LO, lo >> _S32, hi & _LO, hi >> _S32
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LO, (p0 >> _S32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _select(words, which):
    """words uint32[..., 4], which int[...] in 0..3 -> uint64[...]."""
    return np.take_along_axis(words, np.asarray(which)[..., None], axis=-1)[..., 0].astype(np.uint64)


def uniform_positions(seed, offset, cnt, K):
    """int64[N, K]: slot j of query q draws position (word[j & 3] * cnt[q]) >> 32 of its history, from the block at counter
    (q, offset + (j >> 2)), clamped to [0, cnt) as the kernel clamps (a no-op for cnt < 2^32).  Rows with cnt == 0 hold -1."""
    cnt = np.asarray(cnt, np.int64)
    N = cnt.shape[0]
    q = np.arange(N, dtype=np.uint64)[:, None]
    j = np.arange(K, dtype=np.int64)[None, :]
    with np.errstate(over="ignore"):
        hi = np.broadcast_to(_u64(offset), (1, K)) + (j >> 2).astype(np.uint64)              # wraps mod 2^64 like the kernel's
    w = _select(philox4x32_10(seed, q, hi), np.broadcast_to(j & 3, (N, K)))
    idx = ((w * np.maximum(cnt, 0).astype(np.uint64)[:, None]) >> _S32).astype(np.int64)
    idx = np.minimum(np.maximum(idx, 0), np.maximum(cnt, 1)[:, None] - 1)
    return np.where(cnt[:, None] > 0, idx, -1)


def available_lists(item_avail, port_idx, port_len):
    """Per row the list the kernel compacts: ascending item index, available, not among the first min(port_len, W) portfolio
    entries (entries outside [0, n_items), -1 padding included, exclude nothing)."""
    avail = np.flatnonzero(np.asarray(item_avail) != 0).astype(np.int64)
    port_len = np.asarray(port_len, np.int64)
    B = port_len.shape[0]
    port_idx = np.asarray(port_idx, np.int64).reshape(B, -1) if port_idx is not None else np.zeros((B, 0), np.int64)
    W = port_idx.shape[1]
    return [avail[~np.isin(avail, port_idx[b, :max(0, min(int(port_len[b]), W))])] for b in range(B)]


def neg_draw(item_avail, port_idx, port_len, size, upper_u, seed, offset):
    """int64[B, size] item NODE ids (index + upper_u + 1).  Row b reads word k & 3 of the block at counter (b + offset, k >> 2):
    n_avail >= size -> partial Fisher-Yates over the row's list (step k swaps entry k with entry k + (word * (n_avail - k)) >> 32
    and emits it); 0 < n_avail < size -> list[(word * n_avail) >> 32], with replacement; n_avail == 0 -> all zeros."""
    lists = available_lists(item_avail, port_idx, port_len)
    B = len(lists)
    n_av = np.array([len(l) for l in lists], np.int64)
    out = np.zeros((B, size), np.int64)
    if B == 0:
        return out
    k = np.arange(size, dtype=np.int64)[None, :]
    with np.errstate(over="ignore"):
        lo = np.arange(B, dtype=np.uint64)[:, None] + _u64(offset)                           # b + offset wraps mod 2^64
    w = _select(philox4x32_10(seed, lo, (k >> 2).astype(np.uint64)), np.broadcast_to(k & 3, (B, size)))   # [B, size]
    pool = np.zeros((B, max(1, int(n_av.max()))), np.int64)
    for b, l in enumerate(lists):
        pool[b, :len(l)] = l
    # with replacement
    rep = np.flatnonzero((n_av > 0) & (n_av < size))
    if len(rep):
        j = ((w[rep] * n_av[rep].astype(np.uint64)[:, None]) >> _S32).astype(np.int64)
        out[rep] = np.take_along_axis(pool[rep], j, axis=1) + upper_u + 1
    # without replacement: the serial walk over k, all such rows at once
    fy = np.flatnonzero(n_av >= size)
    if len(fy):
        p, n = pool[fy].copy(), n_av[fy]
        r = np.arange(len(fy))
        for kk in range(size):
            span = (n - kk).astype(np.uint64)
            j = kk + ((w[fy, kk] * span) >> _S32).astype(np.int64)
            a, c = p[r, kk].copy(), p[r, j].copy()
            p[r, kk], p[r, j] = c, a
            out[fy, kk] = c + upper_u + 1
    return out


def dropout_threshold(p):
    """uint32(min(p * 2^32, 4294967040)) with every operation in fp32, as the kernel computes it."""
    t = min(np.float32(p) * np.float32(4294967296.0), np.float32(4294967040.0))
    assert type(t) is np.float32
    return np.uint64(int(t))


def dropout_keep(seed, offset, N, K, H, p):
    """bool[N, H, K]: head h of key slot `lane` of instance n is KEPT iff word[h] of the block at counter (n * 64 + lane, offset)
    is >= the threshold.  p <= 0 keeps everything."""
    if np.float32(p) <= 0:
        return np.ones((N, H, K), bool)
    lo = (np.arange(N, dtype=np.uint64) * np.uint64(64))[:, None] + np.arange(K, dtype=np.uint64)[None, :]
    w = philox4x32_10(seed, lo, _u64(offset))                                                # [N, K, 4]
    return np.ascontiguousarray((w[..., :H].astype(np.uint64) >= dropout_threshold(p)).transpose(0, 2, 1))
