"""Error measures, bars and step helpers shared by the parity tests.  Importable without a GPU: the helpers that need the
package or the oracle import them when called."""
import numpy as np


def relerr(a, b):
    """max |a - b| / max |b|: the project's bar for embeddings (BASELINE.json north_star) is stated in this norm."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-12)


def row_relerr(a, b):
    """max_i ||a_i - b_i||_2 / max(||b_i||_2, floor) over the rows of [n, D] arrays.  ``relerr`` divides by the largest entry
    of the whole array: a whole row of small values could be wrong and pass it.  floor = 1e-3 x the median row norm of the
    reference keeps exact-zero rows finite; where more than half of the reference's rows are exactly zero (the memory table a
    few batches after a reset) that median is 0 and the median of the non-zero rows is taken instead."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    a, b = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    if len(b) == 0:
        return 0.0
    norms = np.linalg.norm(b, axis=1)
    med = np.median(norms)
    if med == 0 and (norms > 0).any():
        med = np.median(norms[norms > 0])
    floor = 1e-3 * med
    return float((np.linalg.norm(a - b, axis=1) / np.maximum(np.maximum(norms, floor), 1e-300)).max())


# Per-row bar, beside every embedding / memory ``relerr`` < 1e-4 of the golden comparisons.  Measured first, oracle against the
# reference's fixtures on the CPU (fp32 numpy restatement against torch): the largest per-row error over every g5, g8 and g10
# fixture is 5.3e-7 (g5_step_L2_mem embeddings; memory rows <= 2.6e-7, pending-message rows <= 1e-7, g10 embeddings <= 4.0e-7).
# That is far below the project's 1e-4, so the bar is the project's own figure and not a measured one.
ROW_RTOL = 1e-4


# ---------------------------------------------------------------------------- the step against the oracle (test_gpu_tgn_step.py)
RTOL_EMB = 1e-4      # BASELINE.json north_star: embeddings within 1e-4 relative
# time-encoder gradients are sums of terms scaled by dt ~ 1e7 that cancel to a small remainder: relative to
# max|grad| both the reference's fp32 autograd sum and any re-association of it carry ~1e-3 evaluation noise
RTOL_GRAD_TIME = 3e-3
# oracle comparisons on random parameters: a fc1 pre-activation within rounding distance of 0 flips relu' between
# the two implementations and perturbs every upstream gradient by ~1e-3 (observed once in the D=64 case; all other
# tensors / cases agree to ~1e-5, tools/grad_error_survey.py).  Relative L2 is the metric, with room for one kink.
RTOL_GRAD_ORACLE_L2 = 5e-3   # relative L2 vs the oracle: float-rounding-level differences in the forward flip individual ReLU
                             # units (kinks); two builds of this library that agree with each other to 6e-7 sit at 2.0e-3 and 3.6e-3
                             # against the oracle on the H=4 / uniform configuration.  The reference goldens pin 5e-4 (max norm).
KINK_THR = 2e-5              # |fc1 pre-activation| below this on the oracle side: the ReLU decision could differ between the two
                             # implementations (their forwards agree to ~1e-6) - tests/test_gpu_full_size.py uses the same bound


def _near_kink_roots(ctx, R, K, thr=KINK_THR):
    """Roots whose computation tree (embedding_module.py:110-175 recursion, as cached by the oracle) holds a MergeLayer
    fc1 pre-activation within ``thr`` of zero.  Returns bool[R]."""
    bad = np.zeros(R, bool)

    def walk(c, owners):               # owners[i] = root that instance i of this context belongs to
        if c[0] == "leaf":
            return
        _, l, c_x, c_nb, cache, _, _ = c
        near = (np.abs(cache["z1"]) < thr).any(1)
        np.logical_or.at(bad, owners[near], True)
        walk(c_x, owners)
        walk(c_nb, np.repeat(owners, K))
    walk(ctx, np.arange(R))
    return bad


def _masked_bpr_backward(tgn, ref, emb, rse, rde, rne, B, K, n_neg=3):
    """BPR loss on both sides, its embedding gradient compared (2e-5 of its largest entry), then the backward of BOTH sides
    from its own gradient with the rows of near-kink roots zeroed: a ReLU unit whose pre-activation sits within fp32 noise of
    zero may take the other branch here than in the oracle, and one flipped unit moves every gradient below it by ~1/R
    (measured 1-2.5 % at R = 200, tools/probes/time_grad_error.py).  Such a root is left out ON BOTH SIDES instead of
    loosening the bound for the whole step; a step without one (most) is the plain ``loss.backward()``.
    Returns the oracle's parameter gradients; the product's are in ``p.grad``."""
    import torch
    import pfotgnrec_amd as P
    from oracle import tgn_oracle as T
    loss = P.bpr_loss(emb, B, n_neg)
    (d_emb,) = torch.autograd.grad(loss, emb, retain_graph=True)
    rl, cache = T.bpr_loss(rse, rde.reshape(B, 1, -1), rne.reshape(B, n_neg, -1))
    assert abs(float(loss) - float(rl)) < 1e-5
    ds, dp, dn = T.bpr_loss_backward(cache)
    W = np.concatenate([ds, dp.reshape(B, -1), dn.reshape(n_neg * B, -1)]).astype(np.float32)
    # main.py:321-337 backward; both sides start from their OWN embeddings (which agree to ~1e-6 relative)
    assert np.abs(d_emb.cpu().numpy() - W).max() <= 2e-5 * np.abs(W).max() + 1e-9
    R = W.shape[0]
    bad = _near_kink_roots(ref._ctx, R, K)
    assert bad.sum() < R // 2, bad.sum()
    keep = torch.from_numpy((~bad).astype(np.float32)).to(emb.device)[:, None]
    emb.backward(d_emb * keep)
    W[bad] = 0
    return ref.backward(W)


def _legal_draws(onf, roots, ts, K, L, raw):
    """Turns raw random integers into legal per-query positions, level by level, for both call conventions.

    Product order: one tensor per level (L, L-1, ..., 1), level l covering S_l.  Oracle order: the recursion's call
    order.  Levels are expanded with the oracle's own gather so both agree on the frontier.
    """
    nodes, tss = np.asarray(roots, np.int64), np.asarray(ts, np.float64)
    prod = []
    level_nodes = [(nodes, tss)]
    for i in range(L):
        n_, t_ = level_nodes[-1]
        cnt = np.array([len(onf.find_before(int(a), b)[0]) for a, b in zip(n_, t_)])
        dr = np.where(cnt[:, None] > 0, raw[i] % np.maximum(cnt, 1)[:, None], -1)
        prod.append(dr)
        nb, _, _ = onf.gather_uniform(n_, t_, np.maximum(dr, 0), K)
        level_nodes.append((np.concatenate([n_, nb.flatten()]), np.concatenate([t_, np.repeat(t_, K)])))
    # oracle recursion order for L layers: embed(l, S) = embed(l-1, S) ; sample(S) ; embed(l-1, nbrs(S))
    R = len(nodes)

    def rec(l, lo, hi, level):   # rows [lo, hi) of the product's level tensor `level` (0 = roots level)
        out = []
        if l == 0:
            return out
        out += rec(l - 1, lo, hi, level + 1) if level + 1 < L else []
        out.append(prod[level][lo:hi])
        if level + 1 < L:
            n_level = len(level_nodes[level][0])
            out += rec(l - 1, n_level + lo * K, n_level + hi * K, level + 1)
        return out
    return prod, rec(L, 0, R, 0)


# ---------------------------------------------------------------------------- parameter gradients block by block against float64
# One relative L2 per whole tensor (the bars above) lets a wrong BLOCK through: most tensors are assembled from blocks that
# different kernels and different operands produce, and a block that is a per cent off, or a small block that is entirely
# wrong, moves the tensor's L2 by less than 5e-3.  The measure here is per block, the reference is the oracle evaluated in
# float64 (oracle/tgn_oracle.py, ``dtype=np.float64``: same function, same point, same contract roundings), and the bar
# comes from the reference side alone: the fp32 oracle's own distance from float64 is the noise of one fp32 evaluation of
# this gradient, and the product gets a fixed margin over it.
#
# GRAD_MARGIN = 8 = 4 x 2.  include/pfotgn.h documents the split fp16 contraction at 2^-22 relative error per product against
# 2^-24 for an fp32 product: a factor of 4.  The product contracts with folded composite weights (Wk / Wv folded into the query
# and output sides), which are themselves rounded once before they are used: one more rounding stage, a factor of 2.  No figure
# measured on the product enters the constant or the bar.
GRAD_MARGIN = 8
GRAD_E32_FLOOR = 2.0 ** -23  # e32 below half an fp32 ulp says the fp32 oracle happened to round like float64, not that fp32 can do better
GRAD_BLOCK_FLOOR = 1e-3      # a block's norm is floored at this x ||tensor|| / sqrt(n_blocks): what row_relerr's floor does for rows

_BLOCK_KINDS = (("q_proj_weight", "Wq"), ("k_proj_weight", "Wk"), ("v_proj_weight", "Wv"), ("in_proj_bias", "b_in"),
                ("out_proj.weight", "Wo"), ("fc1.weight", "fc1"), ("weight_ih", "W_ih"), ("weight_hh", "W_hh"),
                ("bias_ih", "b_gru"), ("bias_hh", "b_gru"))


def grad_blocks(name, shape, D, Ef, H):
    """The named sub-blocks of parameter ``name`` (a state_dict name, or the short names Wq, Wk, Wv, b_in, Wo, fc1, W_ih, W_hh)
    as a list of (block name, index tuple); they tile the tensor.  D is the node / memory width, E = 2 D the attention width.

    Wq: head rows x [node | time];  Wk, Wv: head rows x [nbr | Ef | time] (no Ef block at Ef = 0);  b_in: q, k, v thirds;
    Wo: head columns;  fc1: [attention | node];  W_ih: gate rows (r, z, n) x [mem_src | mem_dst | Ef | time];  W_hh and the GRU
    biases: gate thirds;  everything else: the whole tensor."""
    kind = next((k for suffix, k in _BLOCK_KINDS if name.endswith(suffix)), name)
    E = 2 * D
    dh = E // H
    heads = [("h%d" % h, slice(h * dh, (h + 1) * dh)) for h in range(H)]
    gates = [(g, slice(i * D, (i + 1) * D)) for i, g in enumerate("rzn")]
    ef = [("Ef", slice(D, D + Ef))] if Ef > 0 else []
    if kind == "Wq":
        assert tuple(shape) == (E, E), (name, shape)
        return [("%s.%s" % (h, c), (r, s)) for h, r in heads for c, s in (("node", slice(0, D)), ("time", slice(D, E)))]
    if kind in ("Wk", "Wv"):
        assert tuple(shape) == (E, E + Ef), (name, shape)
        cols = [("nbr", slice(0, D))] + ef + [("time", slice(D + Ef, E + Ef))]
        return [("%s.%s" % (h, c), (r, s)) for h, r in heads for c, s in cols]
    if kind == "b_in":
        assert tuple(shape) == (3 * E,), (name, shape)
        return [(t, (slice(i * E, (i + 1) * E),)) for i, t in enumerate("qkv")]
    if kind == "Wo":
        assert tuple(shape) == (E, E), (name, shape)
        return [(h, (slice(None), s)) for h, s in heads]
    if kind == "fc1":
        assert tuple(shape) == (D, E + D), (name, shape)
        return [("attention", (slice(None), slice(0, E))), ("node", (slice(None), slice(E, E + D)))]
    if kind == "W_ih":
        assert tuple(shape) == (3 * D, 3 * D + Ef), (name, shape)
        cols = [("mem_src", slice(0, D)), ("mem_dst", slice(D, 2 * D))] + [("Ef", slice(2 * D, 2 * D + Ef))] * (Ef > 0) \
            + [("time", slice(2 * D + Ef, 3 * D + Ef))]
        return [("%s.%s" % (g, c), (r, s)) for g, r in gates for c, s in cols]
    if kind == "W_hh":
        assert tuple(shape) == (3 * D, D), (name, shape)
        return [(g, (r, slice(None))) for g, r in gates]
    if kind == "b_gru":
        assert tuple(shape) == (3 * D,), (name, shape)
        return [(g, (r,)) for g, r in gates]
    return [("all", (Ellipsis,))]


def block_errors(got, ref64, blocks=None):
    """Per block, ||got - ref||_2 / max(||ref||_2, GRAD_BLOCK_FLOOR x ||ref tensor||_2 / sqrt(n_blocks)), as {block name: error}.
    ``blocks`` as grad_blocks returns them; None is the whole tensor."""
    got, ref = np.asarray(got, np.float64).reshape(np.shape(ref64)), np.asarray(ref64, np.float64)
    blocks = blocks or [("all", (Ellipsis,))]
    floor = GRAD_BLOCK_FLOOR * np.linalg.norm(ref) / np.sqrt(len(blocks))
    return {b: float(np.linalg.norm(got[ix] - ref[ix]) / max(np.linalg.norm(ref[ix]), floor, 1e-300)) for b, ix in blocks}


def grad_block_bar(g32, g64, blocks):
    """(e32, bar) of one tensor: e32 = the fp32 oracle's largest block error against float64, bar = GRAD_MARGIN x max(e32, 2^-23)."""
    e32 = max(block_errors(g32, g64, blocks).values())
    return e32, GRAD_MARGIN * max(e32, GRAD_E32_FLOOR)


def check_grad_blocks(got, g32, g64, D, Ef, H):
    """``got`` {name: product gradient} against the float64 oracle's ``g64`` block by block, at the bar the fp32 oracle's ``g32``
    sets per tensor.  Returns (worst, over): worst = (ratio to the bar, tensor, block, product error, e32) of the block nearest
    to (or furthest over) its bar, over = every (tensor, block, product error, e32, bar) above it.  The caller prints, then
    asserts ``not over``."""
    worst, over = (0.0, None, None, 0.0, 0.0), []
    for name in sorted(got):
        blocks = grad_blocks(name, np.shape(g64[name]), D, Ef, H)
        e32, bar = grad_block_bar(g32[name], g64[name], blocks)
        assert np.isfinite(e32), (name, e32)
        for b, e in block_errors(got[name], g64[name], blocks).items():
            if not e <= bar:
                over.append((name, b, e, e32, bar))
            if not e / bar <= worst[0]:
                worst = (e / bar, name, b, e, e32)
    return worst, over


def fmt_worst_block(worst):
    """The worst block as a FIGURES fragment: tensor, block, product error, e32 and the product's ratio to e32."""
    ratio, name, b, e, e32 = worst
    return "worst block %s[%s] %.3g e32 %.3g ratio %.3g (%.2f of the bar)" % (name, b, e, e32, e / max(e32, GRAD_E32_FLOOR), ratio)


def _relu_sign_disagreements(ctx32, ctx64, R, K):
    """bool[R]: roots whose computation tree holds an fc1 pre-activation that the fp32 and the float64 forward put on different
    sides of zero."""
    out = np.zeros(R, bool)

    def walk(a, b, owners):
        if a[0] == "leaf":
            return
        differ = ((a[4]["z1"] > 0) != (b[4]["z1"] > 0)).any(1)
        np.logical_or.at(out, owners[differ], True)
        walk(a[2], b[2], owners)
        walk(a[3], b[3], np.repeat(owners, K))
    walk(ctx32, ctx64, np.arange(R))
    return out


def f64_twin(ref):
    """A float64 oracle on the graph, features and configuration of the fp32 oracle ``ref``; ``load_state(ref)`` before every
    step puts it at ref's point."""
    import copy
    from oracle import tgn_oracle as T
    t = copy.copy(ref)
    t.dtype = np.float64
    t.node_features = ref.node_features.astype(np.float64)
    t.edge_features = ref.edge_features.astype(np.float64)
    t.load_state(ref)
    assert isinstance(t, T.OracleTGN)
    return t


def _f64_backward(ref64, ref, emb64, B, K, n_neg=3):
    """The float64 side of _masked_bpr_backward: BPR on the float64 embeddings ``emb64`` (src, dst, neg), backward from its own
    gradient with the rows of the roots the FP32 oracle's kink mask names zeroed - the same roots on all sides.  The float64
    run takes its own ReLU branches: on every root the mask keeps they must be the fp32 run's (the mask is 2e-5 wide, the two
    forwards agree to ~1e-6), asserted here.  Returns the float64 parameter gradients."""
    from oracle import tgn_oracle as T
    se, de, ne = emb64
    assert se.dtype == np.float64
    D = se.shape[1]
    _, cache = T.bpr_loss(se, de.reshape(B, 1, D), ne.reshape(B, n_neg, D), dtype=np.float64)
    ds, dp, dn = T.bpr_loss_backward(cache)
    W = np.concatenate([ds, dp.reshape(B, D), dn.reshape(n_neg * B, D)])
    R = W.shape[0]
    bad = _near_kink_roots(ref._ctx, R, K)
    differ = _relu_sign_disagreements(ref._ctx, ref64._ctx, R, K)
    assert not (differ & ~bad).any(), ("float64 and fp32 oracle disagree on a ReLU decision of unmasked roots", np.flatnonzero(differ & ~bad))
    W[bad] = 0
    return ref64.backward(W)
