"""Host side of the wide form of the portfolio-aware top-k (``pfo_recommend_mv_topk_wide``): header and ctypes table, the
workspace arithmetic, ``validate`` beyond 2048 candidates, every ValueError of ``recommend_mv_topk_wide`` without a device, the
dispatcher op's fake, and ``TGN.recommend`` on a CPU model taking the new route up to the point where it asks for a device."""
import os
import re
import types

import numpy as np
import pytest
import torch

import pfotgnrec_amd as P
from pfotgnrec_amd import _lib
from pfotgnrec_amd import recommend as RC
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pfotgn.h")


def _declaration(name):
    """(return type, [argument declarations]) of ``name`` in include/pfotgn.h."""
    text = open(HEADER).read()
    m = re.search(r"^(\w+) %s\(([^;]*)\);" % name, text, re.M)
    assert m, "%s is not declared" % name
    return m.group(1), [a.strip() for a in m.group(2).replace("\n", " ").split(",")]


def _bytes(U, I):
    return _lib.byte_count("pfo_recommend_mv_wide_workspace_bytes", U, I)


def test_header_and_ctypes_table():
    ret, wide = _declaration("pfo_recommend_mv_topk_wide")
    _, bounded = _declaration("pfo_recommend_mv_topk")
    assert ret == "int" and len(wide) == 33 and len(bounded) == 31
    assert wide[:30] == bounded[:30], "the first 30 arguments are pfo_recommend_mv_topk's, same names, same order"
    assert wide[30:] == ["void* workspace", "int64_t workspace_bytes", "void* stream"] and bounded[30] == "void* stream"
    assert _declaration("pfo_recommend_mv_wide_workspace_bytes") == ("int64_t", ["int64_t U", "int32_t I"])
    assert re.search(r"#define PFO_RECOMMEND_MV_WIDE_MAX_ITEMS\s+PFO_RECOMMEND_MAX_ITEMS\b", open(HEADER).read())
    proto, old = _lib.PROTOTYPES["pfo_recommend_mv_topk_wide"], _lib.PROTOTYPES["pfo_recommend_mv_topk"]
    assert len(proto[1]) == 33 and proto[1][:30] == old[1][:30] and proto[0] is old[0]
    assert len(_lib.PROTOTYPES["pfo_recommend_mv_wide_workspace_bytes"][1]) == 2
    lib = _lib.load()
    assert hasattr(lib, "pfo_recommend_mv_topk_wide") and hasattr(lib, "pfo_recommend_mv_wide_workspace_bytes")
    assert lib.pfo_abi_version() == 6
    assert _lib.RECOMMEND_MV_WIDE_MAX_ITEMS == _lib.RECOMMEND_MAX_ITEMS == 65536 and _lib.RECOMMEND_MV_MAX_ITEMS == 2048
    assert P.recommend_mv_topk_wide is P.functional.recommend_mv_topk_wide


def test_workspace_size():
    """36 bytes per user and candidate - y / fused f64, two y-key buffers u64, score f32, two score-key buffers u32 - with the
    users counted in tiles of 16 and the candidates rounded up to 16 (include/pfotgn.h)."""
    layout = lambda U, I: (8 + 8 + 8 + 4 + 4 + 4) * 16 * ((U + 15) // 16) * (16 * ((I + 15) // 16))
    assert _bytes(17, 2100) == layout(17, 2100) == 36 * 32 * 2112
    assert _bytes(512, 65536) == layout(512, 65536) == 36 * 512 * 65536
    for I in (1, 17, 2049, 65536):
        assert _bytes(1, I) > 0
        assert _bytes(1, I) == _bytes(16, I) < _bytes(17, I) == _bytes(32, I)
        sizes = [_bytes(U, I) for U in (1, 2, 15, 16, 17, 31, 33, 100, 1000)]
        assert sizes == sorted(sizes)
    for U in (1, 16, 40):
        sizes = [_bytes(U, I) for I in (1, 2, 16, 17, 500, 2048, 2049, 4097, 65535, 65536)]
        assert sizes == sorted(sizes) and sizes[0] > 0


def _mv(n_stocks):
    return types.SimpleNamespace(returns=np.zeros((2, n_stocks, 3)), upper_u=0, gamma=2.0, lambda_mv=0.5, day_of=None)


def _validate(I, **kw):
    return RC.validate(I + 10, None, [1, 2, 3], 5.0, 3, np.arange(1, I + 1), None, None, None, mv=_mv(5), portfolios=[[], [], []],
                       day_idx=0, **kw)


def test_validate_takes_long_lists_with_mv_and_keeps_the_basket_bounded():
    for I in (2049, 65536):
        q = _validate(I)
        assert isinstance(q, RC.Query) and q.I == I and q.mv is not None and not q.basket
    with pytest.raises(ValueError):
        _validate(65537)
    with pytest.raises(ValueError, match=r"(?s)(basket.*2048|2048.*basket)"):
        _validate(2049, basket=True)
    q = _validate(2048, basket=True)
    assert q.basket and q.I == 2048
    # validate_mv keeps its bound unless told otherwise
    args = dict(U=3, mv=_mv(5), portfolios=[[], [], []], day_idx=0, ts_h=None, scalar_ts=True)
    with pytest.raises(ValueError, match="2048"):
        RC.validate_mv(I=2049, **args)
    assert RC.validate_mv(I=2049, max_items=_lib.RECOMMEND_MV_WIDE_MAX_ITEMS, **args).day_idx.tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="65536"):
        RC.validate_mv(I=65537, max_items=_lib.RECOMMEND_MV_WIDE_MAX_ITEMS, **args)


def test_recommend_mv_topk_wide_validates_then_requires_a_gpu():
    ue, ie = torch.zeros(3, 8), torch.zeros(10, 8)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    good = dict(user_emb=ue, item_emb=ie, k=3, cand_stock=i32(10), returns=torch.zeros(2, 5, 29, dtype=torch.float64),
                day_idx=i32(3), port_idx=i32(3, 4), port_len=i32(3), gamma=2.0, lambda_mv=0.5)
    need = _bytes(3, 10)
    for kw in (dict(k=0), dict(k=65), dict(cand_stock=i32(9)), dict(cand_stock=torch.zeros(10, dtype=torch.int64)),
               dict(returns=torch.zeros(2, 5, 29)), dict(returns=torch.zeros(2, 5, 1, dtype=torch.float64)),
               dict(returns=torch.zeros(2, 5, 129, dtype=torch.float64)), dict(returns=torch.zeros(10, 29, dtype=torch.float64)),
               dict(day_idx=i32(2)), dict(day_idx=torch.zeros(3, dtype=torch.int64)), dict(port_idx=i32(2, 4)),
               dict(port_len=i32(2)), dict(port_idx=None), dict(user_block=i32(2)), dict(n_blocks=3),
               dict(item_ok=torch.ones(4, dtype=torch.uint8)), dict(excl_len=i32(3)), dict(user_emb=torch.zeros(3, 6)),
               dict(user_emb=ue.double()),
               dict(workspace=torch.empty(need - 1, dtype=torch.uint8)),                       # short
               dict(workspace=torch.empty(need, dtype=torch.uint8, device="meta")),            # not where the embeddings live
               dict(workspace=torch.empty(need, dtype=torch.float32)),                         # not bytes
               dict(workspace=torch.empty(2 * need, dtype=torch.uint8)[::2])):                 # not contiguous
        with pytest.raises(ValueError):
            P.recommend_mv_topk_wide(**dict(good, **kw))
    with pytest.raises(ValueError, match="65536"):
        P.recommend_mv_topk_wide(torch.zeros(3, 8), torch.zeros(65537, 8), 3, i32(65537), torch.zeros(2, 5, 3, dtype=torch.float64), i32(3),
                                 None, None, 2.0, 0.5)
    if torch.cuda.is_available():
        # a workspace on the host for embeddings on the device
        dev = lambda t: t.cuda() if isinstance(t, torch.Tensor) else t
        with pytest.raises(ValueError):
            P.recommend_mv_topk_wide(**dict({n: dev(t) for n, t in good.items()}, workspace=torch.empty(need, dtype=torch.uint8)))
    # host tensors: the library is asked, and it has no CPU path - with or without a workspace, beyond the old bound too
    with pytest.raises(_lib.PfoError):
        P.recommend_mv_topk_wide(**good)
    with pytest.raises(_lib.PfoError):
        P.recommend_mv_topk_wide(**dict(good, workspace=torch.empty(need, dtype=torch.uint8)))
    with pytest.raises(_lib.PfoError):
        P.recommend_mv_topk_wide(torch.zeros(3, 8), torch.zeros(2049, 8), 3, i32(2049), torch.zeros(2, 5, 3, dtype=torch.float64), i32(3),
                                 None, None, 2.0, 0.5)


def test_dispatcher_op_fake():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        args = (torch.empty(7, 8), torch.empty(6000, 8), 5, torch.empty(3000, dtype=torch.int32), torch.empty(2, 5, 29, dtype=torch.float64),
                torch.empty(7, dtype=torch.int32), 2.0, 0.5, 2)
        out = torch.ops.pfotgn.recommend_mv_topk_wide(*args)
        old = torch.ops.pfotgn.recommend_mv_topk(*args)
    shapes = lambda ts: [(tuple(t.shape), t.dtype) for t in ts]
    assert shapes(out) == shapes(old) == [((7, 5), torch.int32), ((7, 5), torch.float32), ((7, 5), torch.float64), ((7,), torch.int32)]


def test_recommend_over_2100_items_on_a_cpu_model_asks_for_a_device():
    """The query passes every host check - it is no longer refused for its length - and fails where the device is asked for:
    there is no fallback."""
    g = make_graph(SyntheticConfig("t", 50, 2100, 400, 8, 1, 4, 2), with_prices=False)
    tgn = P.TGN(P.get_neighbor_finder(g.data, False), g.node_features, g.edge_features, "cpu", n_layers=1, n_heads=2, use_memory=True,
                memory_dimension=8, message_function="identity")
    mv = types.SimpleNamespace(returns=torch.zeros(4, 2100, 29, dtype=torch.float64), upper_u=50, gamma=2.0, lambda_mv=0.5,
                               day_of=lambda ts: np.asarray(ts, np.int64) % 4)
    items = np.arange(51, 51 + 2100)
    with pytest.raises(_lib.PfoError):
        tgn.recommend([1, 2, 3], 5.0, 3, items, mv=mv, portfolios=[[0], [], [1, 2]])
    with pytest.raises(ValueError, match="basket"):
        tgn.recommend([1, 2, 3], 5.0, 3, items, mv=mv, portfolios=[[0], [], [1, 2]], basket=True)
