"""Host model (numpy) of what FusedAdam adds to the Adam kernel: the gradient's global L2 norm over element ranges of the flat
buffer, torch.nn.utils.clip_grad_norm_'s coefficient, torch.optim.AdamW's decoupled decay, one AdamW step, and the layout of
torch.optim.Adam's state dict.  fp32 where the device computes in fp32, in the device's order of operations; fp64 where it says so."""
import numpy as np

F32 = np.float32
GRAD_NORM_PARTS = 256           # PFO_GRAD_NORM_PARTS
MAX_RANGES = 16                 # PFO_ADAM_MAX_RANGES
ADAM_BAR = 2e-6                 # tests/test_gpu_kernels.py::test_fused_adam_matches_torch_adam: max |p - p_torch| at lr 1e-3


def elements(lo, hi):
    """Indices of the listed elements, range after range."""
    parts = [np.arange(a, b, dtype=np.int64) for a, b in zip(lo, hi)]
    return np.concatenate(parts) if parts else np.zeros(0, np.int64)


def sumsq64(g, lo, hi):
    """Sum of squares of the listed elements, squares and sum in fp64 (1e20 ** 2 is finite there)."""
    x = np.asarray(g)[elements(lo, hi)].astype(np.float64)
    with np.errstate(all="ignore"):
        return np.float64(np.sum(x * x))


def total_norm(g, lo, hi):
    """total = (float) sqrt(sum): the fp64 square root rounded once to fp32."""
    with np.errstate(all="ignore"):
        return F32(np.sqrt(sumsq64(g, lo, hi)))


def clip_coef(total, max_norm):
    """clip_grad_norm_: clamp(max_norm / (total + 1e-6), max=1) in fp32; a NaN stays a NaN, total = inf gives 0."""
    with np.errstate(all="ignore"):
        c = F32(max_norm) / (F32(total) + F32(1e-6))
    return F32(1.0) if c > F32(1.0) else F32(c)


def decay_factor(lr, weight_decay):
    """float32(1 - lr * weight_decay): formed in double, rounded once (param.mul_(1 - lr * wd))."""
    return F32(1.0 - float(lr) * float(weight_decay))


def prestep(p, g, lo, hi, max_norm, decay, total=None):
    """(p', g', total) after the pre-step over the ranges: g[i] *= coef where max_norm > 0, p[i] *= decay where decay != 1; elements
    outside the ranges unchanged.  ``total``: the norm to use instead of the model's own (the device's, to hold the products to it)."""
    p, g = np.array(p, dtype=F32, copy=True), np.array(g, dtype=F32, copy=True)
    idx = elements(lo, hi)
    if max_norm is not None and max_norm > 0:
        total = total_norm(g, lo, hi) if total is None else F32(total)
        with np.errstate(all="ignore"):
            g[idx] = g[idx] * clip_coef(total, max_norm)
    else:
        total = None
    if F32(decay) != F32(1.0):
        with np.errstate(all="ignore"):
            p[idx] = p[idx] * F32(decay)
    return p, g, total


def adam_update(p, g, m, v, t, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, dtype=np.float32):
    """One Adam update of step count ``t`` (>= 1) in ``dtype`` in the kernel's order (csrc/misc.hip): the lerp form of the first
    moment, bias corrections from fp64 powers.  Returns (p, m, v)."""
    T = dtype
    p, g, m, v = (np.asarray(a, dtype=T) for a in (p, g, m, v))
    b1, b2 = T(betas[0]), T(betas[1])
    bc1 = T(1.0 - float(np.float32(betas[0])) ** t) if T is np.float32 else T(1.0 - betas[0] ** t)
    bc2s = T(np.sqrt(1.0 - float(np.float32(betas[1])) ** t)) if T is np.float32 else T(np.sqrt(1.0 - betas[1] ** t))
    m = m + (g - m) * (T(1.0) - b1)
    v = v * b2 + (T(1.0) - b2) * g * g
    p = p - (T(lr) / bc1) * (m / (np.sqrt(v) / bc2s + T(eps)))
    return p.astype(T), m.astype(T), v.astype(T)


class HostAdamW:
    """clip_grad_norm_ + torch.optim.AdamW over a list of tensors, per-tensor step counts, tensors without a gradient skipped."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, dtype=np.float32):
        self.dtype = dtype
        self.p = [np.array(x, dtype=dtype, copy=True) for x in params]
        self.m = [np.zeros_like(x) for x in self.p]
        self.v = [np.zeros_like(x) for x in self.p]
        self.t = [0] * len(self.p)
        self.lr, self.betas, self.eps, self.wd, self.max_norm = lr, betas, eps, weight_decay, max_grad_norm
        self.last_total = None

    def step(self, grads):
        """``grads``: one array or None per tensor.  The flat layout is the tensors that have a gradient, end to end."""
        live = [i for i, g in enumerate(grads) if g is not None]
        sizes = [self.p[i].size for i in live]
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        flat_p = np.concatenate([self.p[i].reshape(-1) for i in live]).astype(np.float32)
        flat_g = np.concatenate([np.asarray(grads[i], dtype=np.float32).reshape(-1) for i in live])
        new_p, new_g, total = prestep(flat_p, flat_g, [0], [int(off[-1])], self.max_norm, decay_factor(self.lr, self.wd))
        self.last_total = total
        for j, i in enumerate(live):
            self.t[i] += 1
            sl = slice(int(off[j]), int(off[j + 1]))
            p, m, v = adam_update(new_p[sl], new_g[sl], self.m[i].reshape(-1), self.v[i].reshape(-1), self.t[i], self.lr, self.betas, self.eps,
                                  self.dtype)
            self.p[i], self.m[i], self.v[i] = p.reshape(self.p[i].shape), m.reshape(self.p[i].shape), v.reshape(self.p[i].shape)


def torch_state_dict(shapes, steps, exp_avg, exp_avg_sq, group):
    """The layout torch.optim.Adam.state_dict() writes: ``state[i] = {step: f32 scalar tensor, exp_avg, exp_avg_sq}`` for the
    tensors with steps[i] > 0 (index = position in the parameter list), one group with ``params = [0 .. n)``."""
    import torch
    state = {}
    for i, shape in enumerate(shapes):
        if steps[i] > 0:
            state[i] = {"step": torch.tensor(float(steps[i]), dtype=torch.float32),
                        "exp_avg": torch.from_numpy(np.asarray(exp_avg[i], dtype=np.float32).reshape(shape).copy()),
                        "exp_avg_sq": torch.from_numpy(np.asarray(exp_avg_sq[i], dtype=np.float32).reshape(shape).copy())}
    g = dict(group)
    g["params"] = list(range(len(shapes)))
    return {"state": state, "param_groups": [g]}


GROUP_KEYS = ("lr", "betas", "eps", "weight_decay", "max_grad_norm", "params")
