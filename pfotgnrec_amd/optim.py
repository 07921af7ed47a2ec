"""Adam over the TGN's flat parameter buffer: one kernel per step (torch.optim.Adam semantics, main.py:123,389).

torch.optim.Adam keeps one step counter per parameter tensor and skips tensors whose ``.grad`` is None.  The
reference hits that on the first batch after every ``__init_memory__`` (main.py:153): no message is pending, the GRU
is never called (memory_updater.py:38-40) and its four tensors stay one step behind for the rest of the run.  The same
bookkeeping is done here on the host; the device work is still ONE launch (``pfo_adam_step_ranges``: contiguous runs of
tensors with equal step counts).

``weight_decay`` (torch.optim.AdamW's decoupled form) and ``max_grad_norm`` (torch.nn.utils.clip_grad_norm_) put one or two
small launches of csrc/optim.hip in front of that kernel, on the stream the step goes to; ``state_dict()`` / ``load_state_dict()``
speak the layout of torch.optim.Adam / AdamW, so a run resumes and moves between the two optimizers.
"""
import ctypes
import math

import torch

from . import _lib


class _StepCounts(dict):
    """parameter -> steps taken, stored under id(parameter) (hashing a tensor is a Python-level call: ~100 of them per step);
    tensors and ids are both accepted as keys."""
    @staticmethod
    def _k(key):
        return key if isinstance(key, int) else id(key)

    def __getitem__(self, key):
        return dict.__getitem__(self, self._k(key))

    def __setitem__(self, key, value):
        dict.__setitem__(self, self._k(key), value)

    def __contains__(self, key):
        return dict.__contains__(self, self._k(key))

    def get(self, key, default=None):
        return dict.get(self, self._k(key), default)

    def copy(self):
        return _StepCounts(self)


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, tgn, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, zero_grads_in_step=False,
                 overlap_backward=False):
        """``overlap_backward``: for the reference's own loop (main.py:160-394), which reads ``loss.item()`` after every batch.
        ``loss.backward()`` leaves the native backward on a stream of its own and ``step()`` queues the optimizer's kernel behind
        it there, so that ``loss.item()`` waits for the forward only and the host prepares the next batch (candidate draw,
        uploads, launches) while the device is still differentiating; the next forward - and ``state_dict()``, ``tgn.join()`` -
        wait for the step.  Gradients and parameters are IN FLIGHT after ``backward()`` / ``step()`` until then: read ``.grad`` or
        a parameter only behind ``tgn.join()``.  One rank, eager mode; anything else takes the serial order.  ``step()`` goes to
        that stream if and only if the model's newest native backward ran there and no step has consumed it (``tgn.beside``);
        a backward on the caller's stream in between (``bpr_step`` without ``optimizer=``) sends it the serial way.  Out of
        reach: parameter gradients torch autograd itself produces on the caller's stream after the fork.
        ``zero_grads_in_step``: a side-stream step (``step(side=True)``, i.e. ``bpr_step(..., optimizer=)``) also CLEARS the
        gradients it consumed - ``optimizer.zero_grad()`` folded into the optimizer's kernel, for loops that zero the gradients
        right after the step anyway (main.py:388-390 does): the next native backward then clears nothing on its critical path.
        ``.grad`` reads zero after such a step.
        ``weight_decay`` (>= 0): torch.optim.AdamW's decoupled decay - every tensor that takes part in the step is multiplied by
        ``float32(1 - lr * weight_decay)`` (formed in double, rounded once, as ``param.mul_(1 - lr * wd)``) before the Adam update;
        tensors whose ``.grad`` is None are left alone entirely.
        ``max_grad_norm`` (None, or > 0 and finite): ``torch.nn.utils.clip_grad_norm_(params, max_grad_norm, norm_type=2)`` in
        front of the update, where the step runs: ``total`` = the L2 norm of the gradients of the tensors that take part in the
        step, ``coef = min(1, max_grad_norm / (total + 1e-6))`` in fp32, every such gradient multiplied by ``coef`` IN PLACE.
        ``last_grad_norm`` (f32[1] on the device, None before the first clipped step) holds ``total`` of the newest step; the
        device writes it and the library never reads it back - read it behind ``tgn.join()``.  The sum of squares is accumulated
        in fp64: a gradient whose squares overflow fp32 gets a finite norm where torch's fp32 norm is ``inf``.  A non-finite
        gradient gives a non-finite ``total``; the arithmetic above is then applied as written under IEEE rules (``coef`` is 0 or
        NaN, and so are the products).  The sum is taken in a fixed order: the same gradient gives the same bits in every step
        form and on every data-parallel rank (the norm is that of the all-reduced gradient).
        Both live in ``param_groups[0]`` and may be changed between steps.  Clipping puts two small launches
        (``pfo_grad_sumsq_ranges``, ``pfo_grad_prestep_ranges``; decay alone the second) in front of the Adam kernel on the same stream - the caller's, the
        backward's (``overlap_backward``), the library's side stream (``bpr_step(..., optimizer=)``) or the capturing one
        (``GraphedTrainStep``); with both off nothing is launched or allocated for them.  A data-parallel rank with either one on
        does not take the two-bucket ``dp_ordered`` route (a global norm needs the WHOLE reduced gradient before the first
        parameter moves): the step waits for the communication stream and takes the single side step.
        ``state_dict()`` / ``load_state_dict()`` use torch.optim.Adam's layout (see there)."""
        self._check_options(weight_decay, max_grad_norm)
        self.tgn = tgn
        self.zero_grads_in_step = bool(zero_grads_in_step)
        if overlap_backward:
            tgn.overlap_backward = True
        super().__init__(list(tgn.parameters()), dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm))
        self._m = None
        self._v = None
        self._partial = None        # f64[PFO_GRAD_NORM_PARTS]: the norm's partial sums (allocated with the moments when clipping is on)
        self.last_grad_norm = None  # f32[1]: the newest step's gradient norm, written by the device
        self._steps = _StepCounts() # id(parameter) -> steps taken (torch.optim.Adam's state[p]["step"]; ids: hashing a tensor is a Python call)
        self._sorted_views = None   # (the model's views in flat-buffer order, sorted once)

    @staticmethod
    def _check_options(weight_decay, max_grad_norm):
        if not (isinstance(weight_decay, (int, float)) and weight_decay >= 0.0 and math.isfinite(weight_decay)):
            raise ValueError("weight_decay must be a finite number >= 0, got %r" % (weight_decay,))
        if max_grad_norm is not None and not (isinstance(max_grad_norm, (int, float)) and max_grad_norm > 0.0 and math.isfinite(max_grad_norm)):
            raise ValueError("max_grad_norm must be None or a finite number > 0, got %r" % (max_grad_norm,))

    def _alloc_state(self, clip):
        """The moments - and, when clipping is on, the norm's buffers with them: nothing is allocated later (a captured step)."""
        flat = self.tgn.flat_parameters
        if self._m is None or self._m.device != flat.device:
            self._m = torch.zeros_like(flat)
            self._v = torch.zeros_like(flat)
            self._partial, self.last_grad_norm = None, None
        if clip and self._partial is None:
            self._partial = torch.zeros(_lib.GRAD_NORM_PARTS, dtype=torch.float64, device=flat.device)
            self.last_grad_norm = torch.zeros(1, dtype=torch.float32, device=flat.device)

    def _prestep(self, lo, hi, lr, weight_decay, max_grad_norm):
        """Global-norm clipping and decoupled decay over the step's ranges, on the CURRENT stream, in front of the Adam launch."""
        tgn = self.tgn
        clip = max_grad_norm is not None
        decay = 1.0 - lr * float(weight_decay)           # (a Python double; the float argument rounds it once)
        MAXR = _lib.ADAM_MAX_RANGES
        stream = _lib.stream_ptr()
        chunks = []
        for i in range(0, len(lo), MAXR):
            k = min(MAXR, len(lo) - i)
            chunks.append((k, (ctypes.c_int64 * k)(*lo[i:i + k]), (ctypes.c_int64 * k)(*hi[i:i + k])))
        if clip:
            for j, ch in enumerate(chunks):              # the whole norm first: every chunk's elements, in stream order
                _lib.call("pfo_grad_sumsq_ranges", tgn.flat_grad.data_ptr(), *ch, self._partial.data_ptr(), 1 if j else 0, stream)
        for ch in chunks:
            _lib.call("pfo_grad_prestep_ranges", tgn.flat_parameters.data_ptr(), tgn.flat_grad.data_ptr(), *ch,
                      self._partial.data_ptr() if clip else None, float(max_grad_norm) if clip else 0.0, decay,
                      self.last_grad_norm.data_ptr() if clip else None, stream)

    # ------------------------------------------------------------------ torch.optim.Adam's state-dict layout
    def state_dict(self):
        """The layout of ``torch.optim.Adam.state_dict()``: ``state`` keyed by the index of the parameter in ``tgn.parameters()``
        order, each entry ``step`` (a float32 scalar tensor), ``exp_avg`` and ``exp_avg_sq`` in the parameter's shape - copies,
        not views of the flat buffers - for the tensors that have taken a step; ``param_groups[0]`` carries ``lr``, ``betas``,
        ``eps``, ``weight_decay``, ``max_grad_norm`` and ``params``.  Joins first (``tgn.join()``)."""
        tgn = self.tgn
        tgn.join()
        index = {id(p): i for i, p in enumerate(self.param_groups[0]["params"])}
        state = {}
        for p, off, n, shape in tgn._views:
            t = self._steps.get(id(p), 0)
            if t <= 0:
                continue
            if self._m is None:
                m = v = torch.zeros(shape, dtype=torch.float32, device=p.device)
            else:
                m, v = self._m[off:off + n].view(shape), self._v[off:off + n].view(shape)
            state[index[id(p)]] = {"step": torch.tensor(float(t), dtype=torch.float32), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        g = self.param_groups[0]
        group = {k: g[k] for k in ("lr", "betas", "eps", "weight_decay", "max_grad_norm")}
        group["params"] = list(range(len(g["params"])))
        return {"state": dict(sorted(state.items())), "param_groups": [group]}

    def load_state_dict(self, state_dict):
        """A dict written by ``torch.optim.Adam``, ``torch.optim.AdamW`` or ``FusedAdam`` over the same model.  Group keys torch
        writes and this optimizer has no use for (``foreach``, ``capturable``, ``fused`` ...) are ignored; ``amsgrad=True`` and
        ``maximize=True`` are refused.  Step counts are kept PER TENSOR (the GRU's tensors lag one step after
        ``__init_memory__``); a tensor absent from ``state`` has zero moments and step 0.  Joins first (``tgn.join()``)."""
        tgn = self.tgn
        tgn.join()
        groups = state_dict["param_groups"]
        if len(groups) != 1:
            raise ValueError("FusedAdam holds one parameter group, the state dict has %d" % len(groups))
        src = groups[0]
        params = self.param_groups[0]["params"]
        if len(src["params"]) != len(params):
            raise ValueError("the state dict names %d parameters, the model has %d" % (len(src["params"]), len(params)))
        for flag in ("amsgrad", "maximize"):
            if src.get(flag):
                raise ValueError("FusedAdam has no %s: a state dict written with %s=True cannot be loaded" % (flag, flag))
        wd = src.get("weight_decay", self.param_groups[0]["weight_decay"])
        mx = src.get("max_grad_norm", self.param_groups[0]["max_grad_norm"])
        self._check_options(wd, mx)
        by_id = {id(p): (off, n, shape) for p, off, n, shape in tgn._views}
        entries = []
        for key, pos in zip(src["params"], range(len(params))):      # (the dict's own indices, in order, name the positions)
            st = state_dict["state"].get(key)
            if st is None:
                continue
            p = params[pos]
            if id(p) not in by_id:
                raise ValueError("parameter %d has optimizer state but FusedAdam never steps it (it is not in the flat buffer)" % pos)
            off, n, shape = by_id[id(p)]
            if tuple(st["exp_avg"].shape) != shape or tuple(st["exp_avg_sq"].shape) != shape:
                raise ValueError("parameter %d: moments of shape %s, the tensor has %s" % (pos, tuple(st["exp_avg"].shape), shape))
            step = st["step"]
            entries.append((p, off, n, int(round(float(step.item() if torch.is_tensor(step) else step))), st["exp_avg"], st["exp_avg_sq"]))
        flat = tgn.flat_parameters
        if entries or self._m is not None:
            self._m, self._v = torch.zeros_like(flat), torch.zeros_like(flat)
            if self._partial is not None and self._partial.device != flat.device:
                self._partial, self.last_grad_norm = None, None
        steps = _StepCounts()
        for p, off, n, t, m, v in entries:
            self._m[off:off + n].copy_(m.detach().reshape(-1))
            self._v[off:off + n].copy_(v.detach().reshape(-1))
            if t > 0:
                steps[id(p)] = t
        self._steps = steps
        g = self.param_groups[0]
        for k in ("lr", "betas", "eps"):
            if k in src:
                g[k] = tuple(src[k]) if k == "betas" else src[k]
        g["weight_decay"], g["max_grad_norm"] = wd, mx

    def zero_grad(self, set_to_none=True):
        if not set_to_none:
            self.tgn.join()                  # (the clear is a torch kernel on the caller's stream)
        return super().zero_grad(set_to_none=set_to_none)

    # tests / checkpoint restore: one step count for every tensor
    @property
    def _t(self):
        return max(self._steps.values(), default=0)

    @_t.setter
    def _t(self, value):
        self._steps = _StepCounts({id(p): int(value) for p in self.tgn.hot_parameters()})

    def sync_steps(self, taken):
        """Adds ``taken`` steps to every tensor that has a gradient (after replaying a captured step ``taken`` times)."""
        for p in self.tgn.hot_parameters():
            if p.grad is not None:
                self._steps[id(p)] = self._steps.get(id(p), 0) + int(taken)

    def set_steps(self, steps_by_name):
        """Per-tensor step counts (``{parameter name: steps taken}``), e.g. from a torch.optim.Adam state dict."""
        names = dict(self.tgn.named_parameters())
        for k, t in steps_by_name.items():
            self._steps[id(names[k])] = int(t)

    @torch.no_grad()
    def step(self, closure=None, step_dev=None, side=False):
        """``step_dev`` (1-element int32 device tensor): the step counts used are the host's plus that device word and the
        host counters are NOT advanced - for steps captured into a HIP graph, which advances the word itself
        (``sync_steps`` folds it back into the host counters afterwards).
        ``side``: the kernel goes to the library's side stream, behind a backward that ran with ``defer_join``
        (``functional.bpr_step(..., optimizer=self)``); otherwise anything pending there is joined first."""
        beside = self.tgn.beside
        if not side and step_dev is None and beside.takes_step():
            return beside.step(lambda: self._step(closure, None, False))      # behind the backward on ITS stream (overlap_backward)
        return self._step(closure, step_dev, side)

    def _step(self, closure, step_dev, side):
        tgn = self.tgn
        g = self.param_groups[0]
        weight_decay, max_grad_norm = g["weight_decay"], g["max_grad_norm"]
        clip = max_grad_norm is not None
        pre = clip or weight_decay != 0        # (both off: nothing below this line is launched, allocated or branched on for them)
        if pre:
            self._check_options(weight_decay, max_grad_norm)
        if side and (self._m is None or self._m.device != tgn.flat_parameters.device or (clip and self._partial is None)):
            side = False            # the moments are allocated (and cleared) on the caller's stream below: this one step runs there
        if not side:
            tgn.join()
            comm = getattr(tgn, "_comm_pending", None)
            if comm is not None:                     # (a serial step behind allreduce_flat_grad_ordered: an empty shard's route)
                tgn._comm_pending = None
                torch.cuda.current_stream(tgn.flat_parameters.device).wait_stream(comm)
        if tgn.flat_grad is None:
            return None
        _lib.require_gpu(tgn.flat_parameters.device)
        if self._m is None or self._m.device != tgn.flat_parameters.device or (clip and self._partial is None):
            self._alloc_state(clip)
        lo, hi, st = [], [], []
        sv = self._sorted_views
        if sv is None or sv[0] is not tgn._views or len(sv[1]) != len(tgn._views):
            sv = self._sorted_views = (tgn._views, [(p, off, n, id(p)) for p, off, n, _ in sorted(tgn._views, key=lambda v: v[1])])
        steps, inc = self._steps, (1 if step_dev is None else 0)
        for p, off, n, key in sv[1]:
            if p.grad is None:                       # torch.optim.Adam: skipped entirely (no moment decay, no step)
                continue
            t = steps.get(key, 0) + inc
            if inc:
                steps[key] = t
            if lo and hi[-1] == off and st[-1] == t:
                hi[-1] = off + n
            else:
                lo.append(off); hi.append(off + n); st.append(t)
        MAXR = 16
        # the kernel may clear what it read when the ranges cover the whole flat buffer (every tensor has a gradient)
        covered = bool(lo) and lo[0] == 0 and hi[-1] == tgn.flat_parameters.numel() and all(hi[j] == lo[j + 1] for j in range(len(lo) - 1))
        zero_all = bool(side and self.zero_grads_in_step and step_dev is None and covered and len(lo) <= MAXR)
        args = (tgn.flat_parameters.data_ptr(), tgn.flat_grad.data_ptr(), self._m.data_ptr(), self._v.data_ptr())
        hyp = (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]))
        # (clipping / decay: a global norm needs the whole reduced gradient before the first parameter moves - no two-bucket route)
        ordered = (side and getattr(tgn, "dp_ordered", False) and step_dev is None and not pre
                   and 0 < tgn.grad_split < tgn.flat_parameters.numel())
        if ordered:
            # Two buckets in order of first use: [0, split) = time encoder, GRU, layer 1 - the next forward reads them on the
            # caller's stream ~70 us into the step and waits for THIS kernel alone; [split, total) = the top layer's block, whose
            # all-reduce ran beside the backward - stepped behind it, met by the next forward through the side stream's order.
            split = tgn.grad_split
            cut_lo, cut_hi, cut_st = [], [], []
            for a, b, t in zip(lo, hi, st):
                if a < split < b:
                    cut_lo += [a, split]; cut_hi += [split, b]; cut_st += [t, t]
                else:
                    cut_lo.append(a); cut_hi.append(b); cut_st.append(t)
            first = [j for j in range(len(cut_lo)) if cut_hi[j] <= split]
            later = [j for j in range(len(cut_lo)) if cut_lo[j] >= split]
            zflag = 4 if zero_all else 0

            def run(idx, last_bucket):
                for i in range(0, len(idx), MAXR):
                    part = idx[i:i + MAXR]
                    k = len(part)
                    bucket = last_bucket if i + MAXR >= len(idx) else (0 if last_bucket == 1 else 2)
                    _lib.call("pfo_tgn_adam_side_bucket", *args, k, (ctypes.c_int64 * k)(*[cut_lo[j] for j in part]),
                              (ctypes.c_int64 * k)(*[cut_hi[j] for j in part]), (ctypes.c_int32 * k)(*[cut_st[j] for j in part]), *hyp, bucket | zflag)
            if first and later:
                run(first, 1)
                tgn.wait_comm_stream()
                run(later, 2)
                tgn.parameters_changed(refresh=False)
                tgn._grad_zeroed = zero_all
                return None
            tgn.wait_comm_stream()                    # (nothing to cut: the plain side step below, behind the top block's all-reduce)
        elif side and getattr(tgn, "_comm_pending", None) is not None:
            tgn.wait_comm_stream()
        if pre and lo:
            # in front of the Adam launch(es), on the stream they go to, over the same ranges
            if side:
                with _lib.on_stream(tgn.side_stream()):          # behind the backward's end and the collective, as bpr_step queues that
                    self._prestep(lo, hi, hyp[0], weight_decay, max_grad_norm)
            else:
                self._prestep(lo, hi, hyp[0], weight_decay, max_grad_norm)
        for i in range(0, len(lo), MAXR):
            k = min(MAXR, len(lo) - i)
            ranges = (k, (ctypes.c_int64 * k)(*lo[i:i + k]), (ctypes.c_int64 * k)(*hi[i:i + k]), (ctypes.c_int32 * k)(*st[i:i + k]))
            if step_dev is not None:
                _lib.call("pfo_adam_step_ranges_dev", *args, *ranges, step_dev.data_ptr(), *hyp, _lib.stream_ptr())
            elif side and zero_all:
                _lib.call("pfo_tgn_adam_side_bucket", *args, *ranges, *hyp, 4)
                tgn._grad_zeroed = True
            elif side:
                _lib.call("pfo_tgn_adam_side", *args, *ranges, *hyp)
            else:
                _lib.call("pfo_adam_step_ranges", *args, *ranges, *hyp, _lib.stream_ptr())
        if lo:
            # the kernel above wrote the parameters behind torch's back: the model's parameter cache (composite weights, weight
            # images) is rebuilt right here, on the library's side stream behind this kernel - beside the next batch's sampling
            # phase - so that the next forward launches none of it.  (A step being captured rebuilds inside its own forward.)
            tgn.parameters_changed(refresh=tgn.refresh_after_step and step_dev is None and not side)
        return None


def overlap_backward(tgn, optimizer):
    """``FusedAdam(tgn, overlap_backward=True)`` for ANY torch optimizer over ``tgn.parameters()`` (main.py:123 builds
    ``torch.optim.Adam``): ``loss.backward()`` leaves the native backward on a stream of its own, and ``optimizer.step()`` -
    wrapped here - runs its kernels on that stream behind it, so the loop's ``loss.item()`` (main.py:390) waits for the forward
    only and the host prepares the next batch beside the backward.  The next forward, ``state_dict()`` and ``tgn.join()`` wait
    for the step; read ``.grad`` or a parameter from torch only behind ``tgn.join()``.  As with ``FusedAdam``, ``step()`` goes to
    that stream only behind a native backward that ran there and that no step has consumed (``tgn.beside``), else the serial way,
    and parameter gradients torch autograd itself produces after the fork are out of reach.  ``optimizer.zero_grad(set_to_none=
    False)`` joins first (its kernels run on the caller's stream).  Returns the optimizer."""
    tgn.overlap_backward = True
    if isinstance(optimizer, FusedAdam) or getattr(optimizer, "_pfo_overlap", None) is tgn:
        return optimizer
    plain_step, plain_zero = optimizer.step, optimizer.zero_grad

    def step(*args, **kwargs):
        if tgn.beside.takes_step():
            return tgn.beside.step(lambda: plain_step(*args, **kwargs))
        tgn.join()
        return plain_step(*args, **kwargs)

    def zero_grad(set_to_none=True):
        if not set_to_none:
            tgn.join()
        return plain_zero(set_to_none=set_to_none)

    optimizer.step, optimizer.zero_grad, optimizer._pfo_overlap = step, zero_grad, tgn
    return optimizer
