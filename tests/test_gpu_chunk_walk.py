"""The forward-only chunk walk shared by ``TGN.embed_device`` and ``TGN._embed_readonly``: walking the roots in several passes
gives, bit for bit, the embeddings and the state of one pass over all of them."""
import numpy as np
import pytest
import torch

from conftest import has_gpu

import pfotgnrec_amd as P
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]


def test_chunked_forward_only_pass_equals_one_pass_bitwise():
    dev = torch.device("cuda:0")
    cfg = SyntheticConfig("walk", 20, 9, 400, 16, 2, 5, 2)
    g = make_graph(cfg, with_prices=False)
    d = g.data
    tgn = P.TGN(P.get_neighbor_finder(d, uniform=False), g.node_features, g.edge_features, dev, n_layers=2, n_heads=2,
                use_memory=True, memory_dimension=16, message_function="identity", n_neighbors=5)
    tgn.eval()
    tgn.eval_dedup = False
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    rs = np.random.RandomState(5)
    B, n_neg = 4, 5                                                    # R = 4 * (2 + 5) = 28: chunks of 8 -> 8, 8, 8, 4

    def batch(s):
        sl = slice(s, s + B)
        neg = rs.randint(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1, size=B * n_neg)
        return i32(d.sources[sl]), i32(d.destinations[sl]), [i32(neg)], [n_neg], f64(d.timestamps[sl]), i32(d.edge_idxs[sl]), 5

    with torch.no_grad():
        for s in range(200, 260, B):                                   # memory and pending messages to start from
            tgn.embed_device(*batch(s))
        args = batch(260)
        start, step0 = tgn.memory.backup_memory(), tgn._step
        got = {}
        for cap in (8, 1 << 20):
            tgn.memory.restore_memory(start)
            tgn._step = step0
            tgn.eval_chunk_roots = cap
            emb, b = tgn.embed_device(*args)
            assert b == B and tuple(emb.shape) == (28, 16)
            m = tgn.memory
            got[cap] = [t.clone() for t in (emb, m.memory.data, m.last_update.data, m.msg_table, m.msg_time, m.has_msg)]
        assert tgn._step == step0 + 1                                  # one pass; the walk before it took four places
    for name, a, b in zip(("embeddings", "memory", "last_update", "msg_table", "msg_time", "has_msg"), got[8], got[1 << 20]):
        assert torch.equal(a, b), name
    assert bool(got[8][0].abs().sum() > 0) and bool(got[8][5].any())
    tgn.eval_chunk_roots = 8
    step = tgn._step
    users, items = np.arange(1, 6), np.arange(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1)
    ids, scores, n_valid = tgn.recommend(users, float(d.timestamps[300]), 3, items)        # 5 + 9 roots: two passes
    assert tgn._step == step and tuple(ids.shape) == (5, 3) and bool((n_valid == 3).all())
