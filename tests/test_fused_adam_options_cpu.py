"""FusedAdam's weight decay, global-norm clipping and torch-format state dict, as far as they go without a device: the host
model of tests/optim_ref.py against torch itself, the constructor's and the new entries' refusals, the boundary, and the
state dict round trip on a CPU-built model."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
import optim_ref as R

NEW_SYMBOLS = ("pfo_grad_sumsq_ranges", "pfo_grad_prestep_ranges")


def _cpu_tgn(seed=3):
    import pfotgnrec_amd as P
    from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
    torch.manual_seed(seed)
    g = make_graph(SyntheticConfig("t", 50, 10, 400, 8, 1, 4, 2), with_prices=False)
    return P.TGN(P.get_neighbor_finder(g.data, False), g.node_features, g.edge_features, "cpu", n_layers=1, n_heads=2, use_memory=True,
                 memory_dimension=8, message_function="identity")


# ------------------------------------------------------------------ the host model against torch
@pytest.mark.parametrize("wd,max_norm", [(0.01, 0.5), (0.0, 0.5), (0.01, None), (0.1, 1e6)])
def test_host_model_matches_torch_adamw_with_clip_grad_norm(wd, max_norm):
    """Three steps of clip_grad_norm_ + torch.optim.AdamW on CPU tensors against the fp32 host model; tensor 1 has no gradient
    in step 0 (neither decayed, nor counted in the norm, nor stepped: it stays one step behind).  The bar is the Adam
    kernel's own against torch.optim.Adam (tests/test_gpu_kernels.py)."""
    rs = np.random.RandomState(11)
    shapes = [(37, 5), (64,), (3, 7, 2), (1,)]
    p0 = [rs.randn(*s).astype(np.float32) for s in shapes]
    tp = [torch.nn.Parameter(torch.from_numpy(x.copy())) for x in p0]
    opt = torch.optim.AdamW(tp, lr=1e-3, weight_decay=wd)
    host = R.HostAdamW(p0, lr=1e-3, weight_decay=wd, max_grad_norm=max_norm)
    host64 = R.HostAdamW(p0, lr=1e-3, weight_decay=wd, max_grad_norm=max_norm, dtype=np.float64)
    for step in range(3):
        grads = [(rs.randn(*s) * 10.0 ** rs.randint(-3, 2)).astype(np.float32) for s in shapes]
        if step == 0:
            grads[1] = None
        for p, g in zip(tp, grads):
            p.grad = None if g is None else torch.from_numpy(g.copy())
        if max_norm is not None:
            total = torch.nn.utils.clip_grad_norm_(tp, max_norm)
        opt.step()
        host.step(grads)
        host64.step(grads)
        if max_norm is not None:
            assert abs(float(host.last_total) - float(total)) <= 1e-6 * float(total)
            assert (R.clip_coef(host.last_total, max_norm) < 1) == (max_norm < 1e3)          # 0.5 clips, 1e6 does not
    assert host.t == [3, 2, 3, 3]
    assert int(opt.state[tp[1]]["step"]) == 2
    for p, h, h64 in zip(tp, host.p, host64.p):
        assert np.abs(h - p.detach().numpy()).max() < R.ADAM_BAR
        assert np.abs(h64 - p.detach().numpy().astype(np.float64)).max() < R.ADAM_BAR
    if max_norm is None and wd:
        assert np.array_equal(p0[1] * R.decay_factor(1e-3, wd), R.prestep(p0[1], p0[1], [0], [64], None, R.decay_factor(1e-3, wd))[0])


def test_host_model_norm_coefficient_and_ranges():
    rs = np.random.RandomState(2)
    g = rs.randn(50).astype(np.float32)
    p = rs.randn(50).astype(np.float32)
    lo, hi = [3, 10, 20], [7, 10, 31]
    idx = R.elements(lo, hi)
    assert list(idx) == [3, 4, 5, 6] + list(range(20, 31))
    assert R.sumsq64(g, lo, hi) == np.sum(g[idx].astype(np.float64) ** 2)
    tot = R.total_norm(g, lo, hi)
    assert tot.dtype == np.float32 and abs(float(tot) - float(torch.from_numpy(g[idx]).norm())) < 1e-6 * float(tot)
    p2, g2, t2 = R.prestep(p, g, lo, hi, 0.25, np.float32(0.999))
    out = np.setdiff1d(np.arange(50), idx)
    assert np.array_equal(p2[out], p[out]) and np.array_equal(g2[out], g[out])
    assert np.array_equal(g2[idx], g[idx] * R.clip_coef(tot, 0.25)) and np.array_equal(p2[idx], p[idx] * np.float32(0.999))
    # fp64 accumulation: squares that overflow fp32 give a finite norm; inf and NaN go through as IEEE has them
    g[5] = 1e20
    assert np.isfinite(R.total_norm(g, lo, hi)) and float(torch.from_numpy(g[idx]).norm()) == math.inf
    assert R.clip_coef(np.float32(np.inf), 1.0) == 0 and np.isnan(R.clip_coef(np.float32(np.nan), 1.0))
    assert R.clip_coef(np.float32(0.0), 1.0) == 1 and R.clip_coef(np.float32(2.0), 1.0) == np.float32(1.0) / (np.float32(2.0) + np.float32(1e-6))


# ------------------------------------------------------------------ constructor
def test_constructor_takes_and_refuses_the_new_options():
    import pfotgnrec_amd as P
    tgn = _cpu_tgn()
    opt = P.FusedAdam(tgn, weight_decay=0.01)                      # (a TypeError before this feature)
    assert opt.param_groups[0]["weight_decay"] == 0.01 and opt.param_groups[0]["max_grad_norm"] is None
    opt = P.FusedAdam(tgn, lr=1e-3, max_grad_norm=2.5, weight_decay=0)
    assert opt.param_groups[0]["max_grad_norm"] == 2.5 and opt.last_grad_norm is None
    plain = P.FusedAdam(tgn)
    assert plain.param_groups[0]["weight_decay"] == 0.0 and plain.param_groups[0]["max_grad_norm"] is None
    for bad in (dict(weight_decay=-1e-3), dict(weight_decay=float("nan")), dict(weight_decay=float("inf")), dict(max_grad_norm=0.0),
                dict(max_grad_norm=-1.0), dict(max_grad_norm=float("inf")), dict(max_grad_norm=float("nan")), dict(weight_decay="0.1")):
        with pytest.raises(ValueError):
            P.FusedAdam(tgn, **bad)


# ------------------------------------------------------------------ boundary
def test_new_symbols_are_declared_bound_and_built():
    from pfotgnrec_amd import _lib, build
    lib = _lib.load()
    text = open(os.path.join(REPO, "include", "pfotgn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(lib, name) and name in _lib.PROTOTYPES, name
    assert len(_lib.PROTOTYPES["pfo_grad_sumsq_ranges"][1]) == 7 and len(_lib.PROTOTYPES["pfo_grad_prestep_ranges"][1]) == 10
    assert re.search(r"#define\s+PFO_GRAD_NORM_PARTS\s+%d\b" % _lib.GRAD_NORM_PARTS, code) and _lib.GRAD_NORM_PARTS == R.GRAD_NORM_PARTS
    assert re.search(r"#define\s+PFO_ADAM_MAX_RANGES\s+%d\b" % _lib.ADAM_MAX_RANGES, code) and _lib.ADAM_MAX_RANGES == R.MAX_RANGES
    assert lib.pfo_abi_version() == 6 and "optim.hip" in build.SOURCES


def _refusals():
    """(id, entry, arguments, a word of the message).  P stands for a device pointer that is never followed."""
    P, S = 1 << 12, None
    arr = lambda *v: (C.c_int64 * len(v))(*v)
    seventeen = arr(*range(17))
    sumsq = lambda **k: [k.get("grad", P), k.get("n", 2), k.get("lo", arr(0, 8)), k.get("hi", arr(4, 12)), k.get("partial", P), 0, S]
    pre = lambda **k: [k.get("param", P), k.get("grad", P), k.get("n", 2), k.get("lo", arr(0, 8)), k.get("hi", arr(4, 12)), k.get("partial", P),
                       k.get("max_norm", 1.0), k.get("decay", 0.5), k.get("norm_out", P), S]
    return [
        ("sumsq-null-grad", "pfo_grad_sumsq_ranges", sumsq(grad=None), "null buffer"),
        ("sumsq-null-partial", "pfo_grad_sumsq_ranges", sumsq(partial=None), "null buffer"),
        ("sumsq-no-ranges", "pfo_grad_sumsq_ranges", sumsq(n=0), "bad range count"),
        ("sumsq-too-many-ranges", "pfo_grad_sumsq_ranges", sumsq(n=17, lo=seventeen, hi=seventeen), "bad range count"),
        ("sumsq-null-lo", "pfo_grad_sumsq_ranges", sumsq(lo=None), "null range arrays"),
        ("sumsq-lo-above-hi", "pfo_grad_sumsq_ranges", sumsq(lo=arr(0, 13)), "bad range"),
        ("sumsq-negative-lo", "pfo_grad_sumsq_ranges", sumsq(lo=arr(-1, 8)), "bad range"),
        ("prestep-null-grad", "pfo_grad_prestep_ranges", pre(grad=None), "null buffer"),
        ("prestep-null-partial", "pfo_grad_prestep_ranges", pre(partial=None), "null buffer"),
        ("prestep-null-norm-out", "pfo_grad_prestep_ranges", pre(norm_out=None), "null buffer"),
        ("prestep-null-param", "pfo_grad_prestep_ranges", pre(param=None), "null buffer"),
        ("prestep-no-ranges", "pfo_grad_prestep_ranges", pre(n=0), "bad range count"),
        ("prestep-too-many-ranges", "pfo_grad_prestep_ranges", pre(n=17, lo=seventeen, hi=seventeen), "bad range count"),
        ("prestep-null-hi", "pfo_grad_prestep_ranges", pre(hi=None), "null range arrays"),
        ("prestep-lo-above-hi", "pfo_grad_prestep_ranges", pre(lo=arr(5, 8)), "bad range"),
        # (what is not needed may be NULL, but the ranges are still checked)
        ("prestep-no-clip-bad-range", "pfo_grad_prestep_ranges", pre(max_norm=0.0, grad=None, partial=None, norm_out=None, lo=arr(5, 8)), "bad range"),
        ("prestep-no-decay-bad-count", "pfo_grad_prestep_ranges", pre(decay=1.0, param=None, n=-1), "bad range count"),
    ]


@pytest.mark.parametrize("cid,entry,args,word", _refusals(), ids=[c[0] for c in _refusals()])
def test_new_entries_refuse_bad_arguments_without_a_device(cid, entry, args, word):
    from pfotgnrec_amd import _lib
    lib = _lib.load()
    assert getattr(lib, entry)(*args) == -1                               # PFO_ERR_INVALID: refused before any device work
    assert word.encode() in lib.pfo_last_error() and entry.encode() in lib.pfo_last_error(), lib.pfo_last_error()
    with pytest.raises(_lib.PfoError, match=word):
        _lib.call(entry, *args)


def test_nothing_to_do_is_accepted_without_a_device():
    """max_norm <= 0 and decay == 1 with every buffer NULL: valid ranges, nothing queued."""
    from pfotgnrec_amd import _lib
    arr = lambda *v: (C.c_int64 * len(v))(*v)
    assert _lib.load().pfo_grad_prestep_ranges(None, None, 2, arr(0, 8), arr(4, 8), None, 0.0, 1.0, None, None) == 0


# ------------------------------------------------------------------ state dict
def test_fresh_state_dict_is_empty_with_the_group_keys():
    import pfotgnrec_amd as P
    tgn = _cpu_tgn()
    opt = P.FusedAdam(tgn, lr=3e-4, weight_decay=0.02, max_grad_norm=1.5)
    sd = opt.state_dict()
    assert sd["state"] == {} and len(sd["param_groups"]) == 1
    g = sd["param_groups"][0]
    assert set(g) == set(R.GROUP_KEYS)
    assert g["lr"] == 3e-4 and tuple(g["betas"]) == (0.9, 0.999) and g["eps"] == 1e-8 and g["weight_decay"] == 0.02 and g["max_grad_norm"] == 1.5
    assert g["params"] == list(range(len(list(tgn.parameters()))))


def _torch_adam_with_state(tgn, cls=torch.optim.Adam, lagging=(), **kw):
    """A torch optimizer over the model with three steps taken (two on the tensors in ``lagging``) on random gradients."""
    params = list(tgn.parameters())
    opt = cls(params, lr=1e-3, **kw)
    gen = torch.Generator().manual_seed(7)
    hot = {id(p) for p in tgn.hot_parameters()}
    for step in range(3):
        for i, p in enumerate(params):
            skip = id(p) not in hot or (step == 0 and i in lagging)         # (the dead layer_norm never has a gradient)
            p.grad = None if skip else torch.randn(p.shape, generator=gen)
        opt.step()
    for p in params:
        p.grad = None
    return opt


@pytest.mark.parametrize("cls", [torch.optim.Adam, torch.optim.AdamW])
def test_torch_state_dict_loads_and_comes_back_tensor_for_tensor(cls):
    import pfotgnrec_amd as P
    tgn = _cpu_tgn()
    params = list(tgn.parameters())
    hot = {id(p) for p in tgn.hot_parameters()}
    gru = [i for i, p in enumerate(params) if p in tgn._gru_params]
    assert len(gru) == 4
    ref = _torch_adam_with_state(tgn, cls, lagging=gru, weight_decay=0.03).state_dict()
    assert {int(ref["state"][i]["step"]) for i in gru} == {2} and len(ref["state"]) == len(hot)
    opt = P.FusedAdam(tgn, lr=5e-2)
    opt.load_state_dict(ref)
    got = opt.state_dict()
    assert sorted(got["state"]) == sorted(ref["state"])
    for i, st in ref["state"].items():
        assert set(got["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert got["state"][i][k].dtype == torch.float32 and torch.equal(got["state"][i][k], st[k].cpu()), (i, k)
        assert got["state"][i]["step"].dim() == 0 and got["state"][i]["exp_avg"].shape == params[i].shape
    assert all(opt._steps[id(params[i])] == (2 if i in gru else 3) for i in ref["state"])
    g = got["param_groups"][0]
    assert set(g) == set(R.GROUP_KEYS) and g["lr"] == 1e-3 and g["weight_decay"] == 0.03 and g["max_grad_norm"] is None
    # copies, not views of the flat buffers
    got["state"][gru[0]]["exp_avg"].add_(1.0)
    assert torch.equal(opt.state_dict()["state"][gru[0]]["exp_avg"], ref["state"][gru[0]]["exp_avg"])
    # ... and the host model's writer of the layout agrees with torch's
    mine = R.torch_state_dict([tuple(p.shape) for p in params], [opt._steps.get(id(p), 0) for p in params],
                              [ref["state"][i]["exp_avg"].numpy() if i in ref["state"] else None for i in range(len(params))],
                              [ref["state"][i]["exp_avg_sq"].numpy() if i in ref["state"] else None for i in range(len(params))],
                              {k: g[k] for k in R.GROUP_KEYS if k != "params"})
    assert sorted(mine["state"]) == sorted(ref["state"]) and mine["param_groups"][0] == g
    assert all(torch.equal(mine["state"][i][k], ref["state"][i][k]) for i in ref["state"] for k in ("step", "exp_avg", "exp_avg_sq"))
    # the way back: torch takes what FusedAdam wrote
    back = torch.optim.Adam(params, lr=1e-3)
    back.load_state_dict(opt.state_dict())
    assert all(torch.equal(back.state[params[i]]["exp_avg_sq"], ref["state"][i]["exp_avg_sq"]) for i in ref["state"])
    # a tensor absent from ``state`` has zero moments and step 0
    partial = {"state": {k: v for k, v in ref["state"].items() if k != gru[1]}, "param_groups": ref["param_groups"]}
    opt.load_state_dict(partial)
    assert gru[1] not in opt.state_dict()["state"] and opt._steps.get(id(params[gru[1]]), 0) == 0
    off, n = next((off, n) for p, off, n, _ in tgn._views if p is params[gru[1]])
    assert not opt._m[off:off + n].any() and not opt._v[off:off + n].any()


def test_state_dicts_this_optimizer_cannot_honour_are_refused():
    import pfotgnrec_amd as P
    tgn = _cpu_tgn()
    opt = P.FusedAdam(tgn)
    with pytest.raises(ValueError, match="amsgrad"):
        opt.load_state_dict(_torch_adam_with_state(tgn, amsgrad=True).state_dict())
    with pytest.raises(ValueError, match="maximize"):
        opt.load_state_dict(_torch_adam_with_state(tgn, maximize=True).state_dict())
    assert opt.state_dict()["state"] == {}
    sd = _torch_adam_with_state(tgn).state_dict()
    sd["param_groups"][0]["weight_decay"] = -0.1
    with pytest.raises(ValueError, match="weight_decay"):
        opt.load_state_dict(sd)


def test_set_steps_and_t_keep_their_meaning():
    import pfotgnrec_amd as P
    tgn = _cpu_tgn()
    opt = P.FusedAdam(tgn, weight_decay=0.01, max_grad_norm=1.0)
    opt._t = 4
    assert opt._t == 4 and len(opt.state_dict()["state"]) == len(tgn.hot_parameters())
    name = next(n for n, p in tgn.named_parameters() if p in tgn._gru_params)
    opt.set_steps({name: 3})
    steps = sorted(float(s["step"]) for s in opt.state_dict()["state"].values())
    assert steps[0] == 3.0 and steps[1] == 4.0 and steps[-1] == 4.0
