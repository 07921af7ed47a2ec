"""The explanation query behind ``TGN.explain``: ``validate`` checks the arguments on the host alone (no device is asked for),
``assemble`` walks the roots through forward-only passes and lets ``pfo_tgn_explain`` read each pass's workspace - the sampled
neighbours, their edge ids and ages, the attention weights of the top layer[s] - before it goes back to the pool."""
import collections
import ctypes
import operator

import numpy as np
import torch

from . import _lib
from .recommend import _host, _int_vector, _to_dev

MAX_WIDTH = _lib.EXPLAIN_MAX_WIDTH
MAX_HOPS = 2
MAX_NEIGHBORS = _lib.MAX_NEIGHBORS

Query = collections.namedtuple("Query", "U K m hops nodes nodes_h timestamps scalar_ts")


def _index(v, what):
    try:
        return operator.index(v)
    except TypeError:
        raise ValueError("%s must be an integer" % what) from None


def validate(n_nodes, n_layers, default_neighbors, nodes, timestamps, m, hops=1, n_neighbors=None):
    """The arguments of ``TGN.explain`` checked (ValueError) and brought into one form; what lives in device tensors is not
    read back."""
    m, hops = _index(m, "m"), _index(hops, "hops")
    if not 1 <= m <= MAX_WIDTH:
        raise ValueError("m must lie in [1, %d] (got %d)" % (MAX_WIDTH, m))
    if not 1 <= hops <= MAX_HOPS:
        raise ValueError("hops must be 1 or 2 (got %d)" % hops)
    if hops > n_layers:
        raise ValueError("hops = %d needs a model of at least that many layers (n_layers = %d)" % (hops, n_layers))
    if n_neighbors is None:
        n_neighbors = _lib.DEFAULT_NEIGHBORS if default_neighbors is None else default_neighbors
    K = _index(n_neighbors, "n_neighbors")
    if K > MAX_NEIGHBORS:
        raise ValueError("n_neighbors must be at most %d (got %d)" % (MAX_NEIGHBORS, K))
    nodes_h = _int_vector(nodes, "nodes", n_nodes)
    U = int(nodes.shape[0]) if nodes_h is None else int(nodes_h.shape[0])
    ts_h = _host(timestamps)
    ts = timestamps if ts_h is None else ts_h
    if ts.ndim != 0 and tuple(ts.shape) != (U,):
        raise ValueError("timestamps must be a scalar or hold one value per node (%d), got shape %s" % (U, tuple(ts.shape)))
    if ts_h is not None and ts_h.dtype.kind not in "fiu":
        raise ValueError("timestamps must be numbers")
    return Query(U, K, m, hops, nodes, nodes_h, ts, ts.ndim == 0)


def assemble(tgn, q, return_raw=False):
    """The device side of ``TGN.explain`` for a validated query: one forward-only pass and one ``pfo_tgn_explain`` launch per
    chunk of ``eval_chunk_roots`` roots (``Serving._walk_readonly``); the launch writes the chunk's rows of the outputs."""
    dev, U, m, hops, H = tgn.device, q.U, q.m, q.hops, tgn.n_heads
    with torch.no_grad():
        nodes_d = _to_dev(dev, q.nodes if q.nodes_h is None else q.nodes_h, torch.int32)
        ts_d = _to_dev(dev, q.timestamps, torch.float64).reshape(-1)
        ts_d = (ts_d.expand(U) if q.scalar_ts else ts_d).contiguous()
        K, ts_d = tgn._no_neighbours(q.K, ts_d)
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        out = (new((U, m), torch.int32), new((U, m), torch.float64), new((U,), torch.int32), new((U, m), torch.int32),
               new((U, m), torch.float32), new((U, m), torch.int32))
        raw, raw_args = None, [None] * 8
        if return_raw:
            raw = dict(nbr=new((U, K), torch.int32), w=new((U, H, K), torch.float32), dt=new((U, K), torch.float32),
                       eidx=new((U, K), torch.int32))
            raw_args = [raw[n] for n in ("nbr", "w", "dt", "eidx")] + [None] * 4
            if hops == 2:
                raw.update(nbr2=new((U, K, K), torch.int32), w2=new((U, K, H, K), torch.float32), dt2=new((U, K, K), torch.float32),
                           eidx2=new((U, K, K), torch.int32))
                raw_args[4:] = [raw[n] for n in ("nbr2", "w2", "dt2", "eidx2")]

        def launch(call, c0, c1):
            rows = [None if t is None else t[c0:c1].data_ptr() for t in list(out) + raw_args]
            _lib.call("pfo_tgn_explain", ctypes.byref(call.cfg), call.ws.data_ptr(), c1 - c0, K, hops, m, *rows, _lib.stream_ptr())
        tgn._walk_readonly(nodes_d, ts_d, K, launch)
    return out + ((raw,) if return_raw else ())
