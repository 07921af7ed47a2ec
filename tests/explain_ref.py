"""The rule of ``pfo_tgn_explain`` (include/pfotgn.h) restated in numpy, from the raw per-slot tables ``TGN.explain`` returns with
``return_raw=True``: head mean, merge by node, sequential sums, order.  Python loops over ``np.float64`` scalars throughout -
nothing is vectorised, so every sum runs in the order the contract names."""
import numpy as np

F64 = np.float64


def head_mean(w_row, k):
    """p[k] of one row ``w_row`` f32[H, K]: the heads summed in ascending order from 0.0 in fp64, divided by H."""
    s = F64(0.0)
    for h in range(w_row.shape[0]):
        s = s + F64(w_row[h, k])
    return s / F64(w_row.shape[0])


def entries(nbr, w, dt, eidx, nbr2=None, w2=None, dt2=None, eidx2=None):
    """The counting entries of ONE root in ascending slot / path order: [(node, weight f64, age f32, edge id)].
    nbr [K], w [H, K], dt [K], eidx [K]; with the level below (nbr2 [K, K], w2 [K, H, K], dt2 [K, K], eidx2 [K, K]) the
    two-hop paths q = j K + i, weight = one rounded product."""
    K = nbr.shape[0]
    out = []
    for j in range(K):
        if int(nbr[j]) == 0:
            continue
        p1 = head_mean(w, j)
        if nbr2 is None:
            out.append((int(nbr[j]), p1, np.float32(dt[j]), int(eidx[j])))
            continue
        for i in range(K):
            if int(nbr2[j, i]) == 0:
                continue
            out.append((int(nbr2[j, i]), p1 * head_mean(w2[j], i), np.float32(dt2[j, i]), int(eidx2[j, i])))
    return out


def merge(ents):
    """Entries that name one node become one: [(node, weight, count, age, edge id)] - the weight summed sequentially in entry
    order from 0.0, the smallest age with its edge id (strictly smaller replaces: among equal ages the first entry)."""
    acc = {}
    for node, wt, age, e in ents:
        if node not in acc:
            acc[node] = [F64(0.0) + wt, 1, age, e]
        else:
            a = acc[node]
            a[0] = a[0] + wt
            a[1] += 1
            if age < a[2]:
                a[2], a[3] = age, e
    return [(node, a[0], a[1], a[2], a[3]) for node, a in acc.items()]


def rank(merged):
    """weight descending, then age ascending, then node id ascending"""
    return sorted(merged, key=lambda t: (-t[1], t[3], t[0]))


def explain(raw, m, hops=1):
    """The six outputs of ``TGN.explain`` as numpy arrays, from its raw tables (a dict of numpy arrays)."""
    U = raw["nbr"].shape[0]
    node = np.full((U, m), -1, np.int32)
    weight = np.zeros((U, m), np.float64)
    n_valid = np.zeros(U, np.int32)
    count = np.zeros((U, m), np.int32)
    age = np.full((U, m), np.nan, np.float32)
    eidx = np.full((U, m), -1, np.int32)
    for u in range(U):
        below = (raw["nbr2"][u], raw["w2"][u], raw["dt2"][u], raw["eidx2"][u]) if hops == 2 else ()
        rows = rank(merge(entries(raw["nbr"][u], raw["w"][u], raw["dt"][u], raw["eidx"][u], *below)))[:m]
        n_valid[u] = len(rows)
        for s, (v, wt, c, a, e) in enumerate(rows):
            node[u, s], weight[u, s], count[u, s], age[u, s], eidx[u, s] = v, wt, c, a, e
    return node, weight, n_valid, count, age, eidx


def dense(node, weight, n_nodes):
    """The answers scattered into [U, n_nodes]: entry [u, v] = the weight of node v for root u (0 where it is not listed)."""
    out = np.zeros((node.shape[0], n_nodes), np.float64)
    for u in range(node.shape[0]):
        for s in range(node.shape[1]):
            if node[u, s] >= 0:
                out[u, node[u, s]] = weight[u, s]
    return out


def oracle_raw(ctx, hops=1):
    """The raw tables from the context ``OracleTGN._embed(...)[1]`` returns for U roots at the top level: the layer's weights
    ``a`` zeroed on rows without a neighbour (``inv``: the reference attends to the padded slot 0 there and zero-fills the
    output), the sampler's neighbours and edge ids, the dt the time encoder saw; with ``hops=2`` the same of the neighbours'
    instances one level down (``ctx[3]``), reshaped [U, K, ..]."""
    def level(c):
        a = np.array(c[4]["a"])                   # (in the oracle's working dtype: an fp64 oracle's weights stay fp64)
        a[np.asarray(c[4]["inv"])] = 0.0
        nbr, eidx, _ = c[6]
        return np.asarray(nbr, np.int32), a, np.asarray(c[5], np.float32), np.asarray(eidx, np.int32)
    nbr, a, dt, eidx = level(ctx)
    raw = dict(nbr=nbr, w=a, dt=dt, eidx=eidx)
    if hops == 2:
        U, K = nbr.shape
        nbr2, a2, dt2, eidx2 = level(ctx[3])
        raw.update(nbr2=nbr2.reshape(U, K, K), w2=a2.reshape(U, K, a2.shape[1], K), dt2=dt2.reshape(U, K, K),
                   eidx2=eidx2.reshape(U, K, K))
    return raw
