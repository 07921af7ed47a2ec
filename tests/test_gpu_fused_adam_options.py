"""FusedAdam(weight_decay=, max_grad_norm=) and its torch-format state dict through every form of the step: against
clip_grad_norm_ + torch.optim.AdamW on a torch clone, every step form bit for bit against the plain one, two data-parallel ranks,
the options off (nothing new is called, nothing changes), resume from a checkpoint, and the swap with torch.optim.Adam mid-run."""
import copy
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import REPO, has_gpu
import optim_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

import pfotgnrec_amd as P
from pfotgnrec_amd import _lib
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph

DEV = "cuda:0"
LR, WD, Q = 1e-3, 0.1, 3
MODELS = {"A": dict(D=8, L=1, K=4, B=6), "B": dict(D=16, L=2, K=4, B=24)}
NEW = ("pfo_grad_sumsq_ranges", "pfo_grad_prestep_ranges")


@functools.lru_cache(maxsize=None)
def _graph(name):
    m = MODELS[name]
    return make_graph(SyntheticConfig("fa" + name, 300, 25, 5000, m["D"], m["L"], m["K"], 2), with_prices=False)


def _tgn(name, seed=5):
    m, g = MODELS[name], _graph(name)
    torch.manual_seed(seed)
    tgn = P.TGN(P.get_neighbor_finder(g.data, False), g.node_features, g.edge_features, DEV, n_layers=m["L"], n_heads=2, dropout=0.0,
                use_memory=True, memory_dimension=m["D"], message_function="identity", n_neighbors=m["K"])
    tgn.deterministic = True                  # bitwise run-to-run reproducible backward: the forms are compared bit for bit
    tgn.train()
    return tgn


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)


def _embed(tgn, name, step):
    m, d = MODELS[name], _graph(name).data
    B, s = m["B"], 2500 + step * m["B"]
    neg = _t(np.random.RandomState(100 + step).randint(301, 326, size=B * Q), np.int32)
    return tgn.embed_device(_t(d.sources[s:s + B], np.int32), _t(d.destinations[s:s + B], np.int32), [neg], [Q],
                            _t(d.timestamps[s:s + B], np.float64), _t(d.edge_idxs[s:s + B], np.int32), m["K"])


def _one_step(tgn, opt, name, step, fused, before_step=None):
    emb, b = _embed(tgn, name, step)
    if fused:
        P.bpr_step(tgn, emb, b, Q, optimizer=opt)
    else:
        P.bpr_loss(emb, b, Q).backward()
        if before_step is not None:
            before_step()
        opt.step()
    opt.zero_grad(set_to_none=True)


def _snapshot(tgn, opt):
    tgn.join()
    torch.cuda.synchronize()
    views = sorted(tgn._views, key=lambda v: v[1])
    return dict(params=tgn.flat_parameters.detach().cpu().numpy().copy(),
                m=None if opt._m is None else opt._m.cpu().numpy().copy(), v=None if opt._v is None else opt._v.cpu().numpy().copy(),
                steps=[opt._steps.get(id(p), 0) for p, _, _, _ in views], memory=tgn.memory.memory.detach().cpu().numpy().copy())


def _run(name, form, first=0, n_steps=3, tgn=None, opt=None, **kw):
    """``n_steps`` steps of one form on a fresh model (or the one given): the snapshot, with the norm after every step."""
    tgn = tgn or _tgn(name)
    if opt is None:
        opt = P.FusedAdam(tgn, lr=LR, zero_grads_in_step=(form == "fused_zero"), overlap_backward=(form == "overlap"), **kw)
    norms = []
    for step in range(first, first + n_steps):
        _one_step(tgn, opt, name, step, fused=form in ("fused", "fused_zero"))
        if opt.param_groups[0]["max_grad_norm"] is not None:
            tgn.join()
            norms.append(float(opt.last_grad_norm.item()))
    out = _snapshot(tgn, opt)
    out.update(norms=norms, tgn=tgn, opt=opt)
    return out


def _same(a, b, keys=("params", "m", "v", "steps", "memory", "norms")):
    return all(np.array_equal(a[k], b[k]) for k in keys)


@functools.lru_cache(maxsize=None)
def _first_norm(name):
    """The first step's gradient norm, measured: the bound that clips it and the one that never does are chosen from it."""
    tgn = _tgn(name)
    emb, b = _embed(tgn, name, 0)
    P.bpr_loss(emb, b, Q).backward()
    total = float(torch.nn.utils.clip_grad_norm_([p for p in tgn.parameters() if p.grad is not None], 1e30))
    assert total > 0
    return total


@functools.lru_cache(maxsize=None)
def _plain(name, clip_scale):
    kw = dict(weight_decay=WD)
    if clip_scale is not None:
        kw["max_grad_norm"] = clip_scale * _first_norm(name)
    out = _run(name, "plain", **kw)
    out.pop("tgn"); out.pop("opt")
    return out


# ------------------------------------------------------------------ against torch
@pytest.mark.parametrize("name", list(MODELS))
def test_three_steps_against_clip_grad_norm_and_adamw(name):
    """The product's own gradient goes into the .grad of a torch clone of the parameters after every native backward; the clone
    is stepped by clip_grad_norm_ + torch.optim.AdamW.  Right after __init_memory__ the GRU's tensors have no gradient: neither
    decayed, nor counted in the norm, nor stepped."""
    tgn = _tgn(name)
    max_norm = 0.5 * _first_norm(name)
    opt = P.FusedAdam(tgn, lr=LR, weight_decay=WD, max_grad_norm=max_norm)
    hot = sorted(tgn._views, key=lambda v: v[1])
    clone = [torch.nn.Parameter(p.detach().clone()) for p, _, _, _ in hot]
    ref = torch.optim.AdamW(clone, lr=LR, weight_decay=WD)
    gru = [i for i, v in enumerate(hot) if v[0] in tgn._gru_params]
    totals, missing = [], []

    def torch_side():
        tgn.join()
        missing.append([i for i, v in enumerate(hot) if v[0].grad is None])
        for c, v in zip(clone, hot):
            c.grad = None if v[0].grad is None else v[0].grad.detach().clone()
        totals.append(float(torch.nn.utils.clip_grad_norm_(clone, max_norm)))
        ref.step()

    gru_before = torch.cat([hot[i][0].detach().reshape(-1) for i in gru]).clone()
    for step in range(3):
        _one_step(tgn, opt, name, step, fused=False, before_step=torch_side)
        tgn.join()
        got = float(opt.last_grad_norm.item())
        print("model %s step %d: norm %.9g (torch %.9g), bound %.9g" % (name, step, got, totals[-1], max_norm))
        assert abs(got - totals[-1]) <= 1e-6 * totals[-1]
        if step == 0:
            assert missing[0] == gru and R.clip_coef(got, max_norm) < 1
            assert torch.equal(torch.cat([hot[i][0].detach().reshape(-1) for i in gru]), gru_before)        # not decayed
    assert missing[1] == [] and missing[2] == []
    worst = max(float((c.detach() - v[0].detach()).abs().max()) for c, v in zip(clone, hot))
    print("model %s: max |p - p_torch| = %.3g" % (name, worst))
    assert worst < R.ADAM_BAR
    assert [opt._steps[v[0]] for v in hot] == [2 if i in gru else 3 for i in range(len(hot))]
    assert [int(ref.state[c]["step"]) for c in clone] == [2 if i in gru else 3 for i in range(len(hot))]


@pytest.mark.parametrize("name", list(MODELS))
def test_a_bound_that_never_binds_changes_nothing(name):
    clipped, loose, free = _plain(name, 0.5), _plain(name, 50.0), _plain(name, None)
    assert R.clip_coef(clipped["norms"][0], 0.5 * _first_norm(name)) < 1
    assert all(R.clip_coef(n, 50.0 * _first_norm(name)) == 1 for n in loose["norms"])
    assert _same(loose, free, keys=("params", "m", "v", "steps", "memory"))
    assert not np.array_equal(clipped["params"], free["params"])
    assert clipped["norms"][0] == loose["norms"][0]                          # (the same first gradient, the same bits)


# ------------------------------------------------------------------ the step forms
@pytest.mark.parametrize("form", ["fused", "fused_zero", "overlap"])
@pytest.mark.parametrize("name", list(MODELS))
def test_step_forms_equal_the_plain_form_bit_for_bit(name, form):
    """bpr_step(..., optimizer=) (pre-step and Adam on the library's side stream), the same with the gradients cleared by the Adam
    kernel behind the pre-step's scaling, and overlap_backward (both on the backward's stream): parameters, moments, step counts,
    memory and the norm of every step equal the plain loss.backward(); opt.step()."""
    got = _run(name, form, weight_decay=WD, max_grad_norm=0.5 * _first_norm(name))
    assert _same(got, _plain(name, 0.5))
    assert R.clip_coef(got["norms"][0], 0.5 * _first_norm(name)) < 1
    if form == "fused_zero":
        assert not got["tgn"].flat_grad.any()


@pytest.mark.parametrize("kw", [dict(weight_decay=WD), dict(max_grad_norm=1e-3), dict(weight_decay=WD, max_grad_norm=1e-3)],
                         ids=["decay", "clip", "both"])
def test_graph_replay_equals_its_eager_step(kw):
    """GraphedTrainStep: the two launches are captured on the capturing stream in front of the device-counted Adam kernel;
    nothing is allocated during capture (the buffers come with the moments, in the warm-up steps).  Lockstep replay against
    the same step queued kernel by kernel: parameters, moments, gradient (scaled in place) and norm bit for bit."""
    from pfotgnrec_amd.rand_edge_sampler import item_availability, DeviceNegativeSampler
    name = "B"
    m, g = MODELS[name], _graph(name)
    d, B = g.data, MODELS[name]["B"]
    sides = []
    for _ in range(2):
        tgn = _tgn(name, seed=31)
        opt = P.FusedAdam(tgn, lr=LR, **kw)
        sampler = DeviceNegativeSampler(item_availability(d.destinations, g.upper_u, 25), g.upper_u, DEV, seed=1)
        arrs = (_t(d.sources, np.int32), _t(d.destinations, np.int32), _t(d.timestamps, np.float64), _t(d.edge_idxs, np.int32),
                _t(g.portfolio_idx, np.int32), _t(g.portfolio_len, np.int32))
        gs = P.GraphedTrainStep(tgn, opt, sampler, B, m["K"], n_neg=Q, port_width=arrs[4].shape[1])
        sides.append((tgn, opt, gs, arrs))
    batch = lambda arrs, s: tuple(a[s:s + B] for a in arrs) + (None,)
    (tA, oA, gA, aA), (tB, oB, gB, aB) = sides
    gA.capture(*batch(aA, 2400), warmup=2)
    gB.capture(*batch(aB, 2400), warmup=2)
    clip = "max_grad_norm" in kw
    assert (oA._partial is not None) == clip and (oA.last_grad_norm is not None) == clip
    held = (oA._partial, oA.last_grad_norm)
    for k in range(3):
        with torch.no_grad():                                  # lockstep: A <- B
            tA.flat_parameters.copy_(tB.flat_parameters)
            oA._m.copy_(oB._m); oA._v.copy_(oB._v)
            tA.memory.restore_memory(tB.memory.backup_memory()); tA.memory._any_msg = True
            gA.rng_pos.copy_(gB.rng_pos); gA.adam_t.copy_(gB.adam_t)
        before = tB.flat_parameters.clone()
        la = float(gA(*batch(aA, 2424 + k * B)))
        lb = float(gB.eager(*batch(aB, 2424 + k * B)))
        torch.cuda.synchronize()
        assert la == lb
        assert torch.equal(tA.flat_grad, tB.flat_grad)
        assert torch.equal(tA.flat_parameters, tB.flat_parameters) and not torch.equal(before, tB.flat_parameters)
        assert torch.equal(oA._m, oB._m) and torch.equal(oA._v, oB._v)
        if clip:
            assert torch.equal(oA.last_grad_norm, oB.last_grad_norm) and float(oA.last_grad_norm.item()) > 1e-3       # it clipped
    assert held[0] is oA._partial and held[1] is oA.last_grad_norm        # (the same buffers: nothing was allocated on the way)
    assert gA.finish() == 3 and gB.finish() == 3


# ------------------------------------------------------------------ options off
def test_options_off_call_nothing_new_and_change_nothing(monkeypatch):
    from pfotgnrec_amd.rand_edge_sampler import item_availability, DeviceNegativeSampler
    called = []
    plain_call = _lib.call

    def recorder(name, *args):
        called.append(name)
        return plain_call(name, *args)
    monkeypatch.setattr(_lib, "call", recorder)
    name = "A"
    runs = {form: _run(name, form) for form in ("plain", "fused", "fused_zero", "overlap")}
    explicit = _run(name, "plain", weight_decay=0.0, max_grad_norm=None)
    g, m = _graph(name), MODELS[name]
    d, B = g.data, MODELS[name]["B"]
    tgn = _tgn(name)
    opt = P.FusedAdam(tgn, lr=LR)
    sampler = DeviceNegativeSampler(item_availability(d.destinations, g.upper_u, 25), g.upper_u, DEV, seed=1)
    arrs = (_t(d.sources, np.int32), _t(d.destinations, np.int32), _t(d.timestamps, np.float64), _t(d.edge_idxs, np.int32),
            _t(g.portfolio_idx, np.int32), _t(g.portfolio_len, np.int32))
    gs = P.GraphedTrainStep(tgn, opt, sampler, B, m["K"], n_neg=Q, port_width=arrs[4].shape[1])
    gs.capture(*(a[2400:2400 + B] for a in arrs), warmup=1)
    gs(*(a[2406:2406 + B] for a in arrs))
    gs.finish()
    assert "pfo_adam_step_ranges" in called and "pfo_tgn_adam_side" in called and "pfo_adam_step_ranges_dev" in called
    assert not [c for c in called if c in NEW]
    for form, r in runs.items():
        assert r["opt"]._partial is None and r["opt"].last_grad_norm is None
        assert _same(r, runs["plain"]), form
    assert _same(explicit, runs["plain"])
    # ... and switched on between two steps through param_groups, they are called
    opt2 = runs["plain"]["opt"]
    opt2.param_groups[0]["max_grad_norm"] = 1e-3
    _run(name, "fused", first=3, n_steps=1, tgn=runs["plain"]["tgn"], opt=opt2)
    assert [c for c in called if c in NEW] == list(NEW) and float(opt2.last_grad_norm.item()) > 1e-3
    opt2.param_groups[0]["weight_decay"] = -1.0
    with pytest.raises(ValueError):
        _run(name, "plain", first=4, n_steps=1, tgn=runs["plain"]["tgn"], opt=opt2)


# ------------------------------------------------------------------ resume and swap
@pytest.mark.parametrize("name", list(MODELS))
def test_resume_from_a_checkpoint_is_bitwise(name, tmp_path):
    """Five steps uninterrupted against three steps, a checkpoint written with torch.save (model, optimizer, memory), fresh
    objects that load it, and two more steps."""
    kw = dict(weight_decay=WD, max_grad_norm=0.5 * _first_norm(name))
    whole = _run(name, "fused", n_steps=5, **kw)
    head = _run(name, "fused", n_steps=3, **kw)
    sd = head["opt"].state_dict()
    assert sd["param_groups"][0]["max_grad_norm"] == kw["max_grad_norm"] and sd["param_groups"][0]["weight_decay"] == WD
    torch.save(dict(model=head["tgn"].state_dict(), optimizer=sd, memory=head["tgn"].memory.backup_memory()), tmp_path / "ckpt.pt")
    ckpt = torch.load(tmp_path / "ckpt.pt", weights_only=False)
    tgn = _tgn(name, seed=77)                                                # (other initial parameters: everything comes from the file)
    opt = P.FusedAdam(tgn, lr=9.0)
    tgn.load_state_dict(ckpt["model"])
    opt.load_state_dict(ckpt["optimizer"])
    tgn.memory.restore_memory(ckpt["memory"])
    assert opt.param_groups[0]["lr"] == LR and opt.param_groups[0]["max_grad_norm"] == kw["max_grad_norm"]
    tail = _run(name, "fused", first=3, n_steps=2, tgn=tgn, opt=opt)
    assert _same(tail, whole, keys=("params", "m", "v", "steps", "memory"))
    assert tail["norms"] == whole["norms"][3:]
    assert sorted(set(whole["steps"])) == [4, 5]                             # (the GRU's four tensors lag one step)


def test_swap_with_torch_adam_mid_run():
    """Two steps under torch.optim.Adam, its state dict into FusedAdam, the third step under each from the same state; then
    FusedAdam's state dict back into a torch.optim.Adam and the fourth step under each."""
    name = "B"
    tgn = _tgn(name)
    adam = torch.optim.Adam(tgn.parameters(), lr=LR)
    for step in range(2):
        _one_step(tgn, adam, name, step, fused=False)
    fused = P.FusedAdam(tgn, lr=LR)
    fused.load_state_dict(copy.deepcopy(adam.state_dict()))
    assert sorted(set(fused._steps.values())) == [1, 2]

    def both(step, first, second):
        """Step ``step`` under ``first``, then - from the same parameters and memory - under ``second``; the worst difference."""
        tgn.join()
        params, mem = tgn.flat_parameters.detach().clone(), tgn.memory.backup_memory()
        _one_step(tgn, second, name, step, fused=False)
        tgn.join()
        theirs = tgn.flat_parameters.detach().clone()
        with torch.no_grad():
            tgn.flat_parameters.copy_(params)
        tgn.parameters_changed()
        tgn.memory.restore_memory(mem)
        _one_step(tgn, first, name, step, fused=False)
        tgn.join()
        return float((tgn.flat_parameters.detach() - theirs).abs().max()), float((tgn.flat_parameters.detach() - params).abs().max())
    diff, moved = both(2, fused, adam)
    print("swap torch -> fused: max |p_fused - p_torch| = %.3g (the step moved %.3g)" % (diff, moved))
    assert diff < R.ADAM_BAR and moved > 10 * R.ADAM_BAR
    back = torch.optim.Adam(tgn.parameters(), lr=LR)
    back.load_state_dict(fused.state_dict())                                 # (no error: torch's own layout)
    assert sorted({int(s["step"]) for s in back.state.values()}) == [2, 3]
    fused2 = P.FusedAdam(tgn, lr=LR)
    fused2.load_state_dict(fused.state_dict())
    diff, moved = both(3, fused2, back)
    print("swap fused -> torch: max |p_fused - p_torch| = %.3g (the step moved %.3g)" % (diff, moved))
    assert diff < R.ADAM_BAR and moved > 10 * R.ADAM_BAR


# ------------------------------------------------------------------ data parallel
DP_MAX_NORM = 1e-3


def _dp_rank(rank, world, port, out_dir, ordered, tag):
    sys.path.insert(0, REPO)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    from pfotgnrec_amd.distributed import init_from_env, allreduce_flat_grad, allreduce_flat_grad_ordered, broadcast_parameters
    init_from_env(backend="gloo")
    name = "B"
    tgn = _tgn(name)
    tgn.set_data_parallel(rank, world)
    tgn.dp_bucketed = tgn.dp_ordered = ordered
    broadcast_parameters(tgn.flat_parameters, world)
    opt = P.FusedAdam(tgn, lr=LR, weight_decay=WD, max_grad_norm=DP_MAX_NORM)
    norms = []
    for step in range(3):
        emb, b = _embed(tgn, name, step)
        P.bpr_step(tgn, emb, b, Q, optimizer=opt,
                   collective=(lambda: allreduce_flat_grad_ordered(tgn, world)) if ordered else (lambda: allreduce_flat_grad(tgn.flat_grad, world)))
        tgn.join()
        norms.append(float(opt.last_grad_norm.item()))
        opt.zero_grad(set_to_none=True)
    snap = _snapshot(tgn, opt)
    np.savez(os.path.join(out_dir, "%s_w%d_r%d.npz" % (tag, world, rank)), norms=np.float32(norms), **snap)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _dp_spawn(tmp_path, *groups):
    """Every (world, port, ordered, tag) group at once - at most three processes in all; the ranks' results, group by group."""
    ctx = mp.get_context("spawn")
    assert sum(g[0] for g in groups) <= 3
    procs = [ctx.Process(target=_dp_rank, args=(r, world, port, str(tmp_path), ordered, tag)) for world, port, ordered, tag in groups
             for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
        assert p.exitcode == 0
    return [[np.load(tmp_path / ("%s_w%d_r%d.npz" % (tag, world, r))) for r in range(world)] for world, _, _, tag in groups]


def test_two_data_parallel_ranks_clip_by_the_norm_of_the_reduced_gradient(tmp_path):
    """Two ranks on one GPU (gloo) against one rank at the same global batch: the norm is that of the all-reduced gradient, so
    the replicas hold the same bits; with dp_ordered requested the two-bucket route is not taken (a global norm needs the whole
    gradient) and the result equals the non-ordered run bit for bit."""
    port = 29450 + (os.getpid() % 100)
    (one,), (r0, r1) = _dp_spawn(tmp_path, (1, port, False, "plain"), (2, port + 1, False, "plain"))
    ((o0, o1),) = _dp_spawn(tmp_path, (2, port + 2, True, "ordered"))
    keys = ("params", "m", "v", "steps", "memory", "norms")
    assert _same(r0, r1, keys) and _same(o0, o1, keys)                       # bit-identical replicas
    assert _same(r0, o0, keys)                                               # ordered requested == not requested
    assert all(n > DP_MAX_NORM for n in one["norms"]) and np.isfinite(one["params"]).all()       # every step clipped
    rel = lambda a, b: np.abs(a.astype(np.float64) - b).max() / (np.abs(b).max() + 1e-12)
    assert abs(float(r0["norms"][0]) - float(one["norms"][0])) < 1e-4 * float(one["norms"][0])    # step 0: identical inputs
    assert rel(r0["params"], one["params"]) < 1e-2 and list(r0["steps"]) == list(one["steps"])
