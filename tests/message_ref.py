"""Host model of the step with the MLP message function (modules/message_function.py:13-26): the oracle of
oracle/tgn_oracle.py with Linear(Mr, Mr // 2) -> ReLU -> Linear(Mr // 2, message_dimension) between the ``last`` aggregator and
the GRU cell, forward and backward, in the oracle's working dtype (fp32 or float64).

Raw messages and stored memory are constants: gradients reach the MLP's four tensors and the GRU's and go no
further down.  The MLP runs lazily on every node that holds a pending message and again on the positives when their memory is
persisted - with the same parameters and the same rows, so the persisted rows are the lazy ones."""
import numpy as np

from oracle import tgn_oracle as T

f32 = np.float32
MLP = "message_function.mlp."
ALIAS = "message_function.layers."
GRU = "memory_updater.memory_updater."
MLP_NAMES = [MLP + "0.weight", MLP + "0.bias", MLP + "2.weight", MLP + "2.bias"]


def mlp_forward(x, W1, b1, W2, b2, dtype=f32):
    """-> (message [n, message_dimension], (x, pre-activation, hidden))."""
    pre = (x @ W1.T + b1).astype(dtype)
    hid = np.maximum(pre, 0).astype(dtype)
    return (hid @ W2.T + b2).astype(dtype), (x, pre, hid)


def mlp_backward(cache, d_out, W2, mask=None):
    """Parameter gradients of the MLP from d loss / d message.  ``mask`` bool[n, hidden]: the ReLU decisions to differentiate
    with (None: the forward's own, pre-activation > 0)."""
    x, pre, hid = cache
    if mask is None:
        mask = pre > 0
    d_hid = (d_out @ W2) * mask
    return {"2.weight": d_out.T @ hid, "2.bias": d_out.sum(0), "0.weight": d_hid.T @ x, "0.bias": d_hid.sum(0)}, d_hid


def gru_input_backward(cache, d_hn, W_ih, dtype=f32):
    """d loss / d (GRU input x) = dgi W_ih: the one gradient oracle.gru_cell_backward does not return (the identity message
    function's input is a constant)."""
    x, h, r, z, n, ghn = cache
    dn = d_hn * (1 - z)
    dz = d_hn * (h - n)
    dpre_n = dn * (1 - n * n)
    dpre_r = dpre_n * ghn * r * (1 - r)
    dpre_z = dz * z * (1 - z)
    dgi = np.concatenate([dpre_r, dpre_z, dpre_n], 1).astype(dtype)
    return (dgi @ W_ih).astype(dtype), dgi


class MlpOracleTGN(T.OracleTGN):
    """OracleTGN with message_function="mlp".  ``params`` by state_dict names; the ``message_function.layers.*`` aliases of a
    reference state dict are dropped (they are the same tensors as ``message_function.mlp.*``)."""

    def __init__(self, neighbor_finder, node_features, edge_features, params, n_layers, n_heads, dtype=f32):
        params = {k: v for k, v in params.items() if not k.startswith(ALIAS)}
        assert all(n in params for n in MLP_NAMES)
        super().__init__(neighbor_finder, node_features, edge_features, params, n_layers, n_heads, use_memory=True, dtype=dtype)
        self._mlp_ctx = None

    def _mlp(self):
        return tuple(self.P[n] for n in MLP_NAMES)

    def _get_updated_memory(self):
        ids, msgs, ts = self._aggregate_last(np.arange(self.n_nodes))
        mem, lu = self.memory.copy(), self.last_update.copy()
        cache, self._mlp_ctx = None, None
        if len(ids) > 0:
            assert (self.last_update[ids] <= ts).all(), "Trying to update memory to time in the past"
            x, self._mlp_ctx = mlp_forward(msgs, *self._mlp(), dtype=self.dtype)
            hn, cache = T.gru_cell(x, mem[ids], *self._gru(), dtype=self.dtype)
            mem[ids] = hn
            lu[ids] = ts
        return mem, lu, (ids, cache)

    def _update_memory(self, positives):
        ids, msgs, ts = self._aggregate_last(positives)
        if len(ids) == 0:
            return
        assert (self.last_update[ids] <= ts).all(), "Trying to update memory to time in the past"
        h = self.memory[ids]
        self.last_update[ids] = ts
        x, _ = mlp_forward(msgs, *self._mlp(), dtype=self.dtype)
        self.memory[ids], _ = T.gru_cell(x, h, *self._gru(), dtype=self.dtype)

    # what the last step's MLP saw: node ids (ascending), hidden pre-activations and activations [n_ids, hidden]
    def mlp_rows(self):
        if self._mlp_ctx is None:
            return np.zeros(0, np.int64), None, None
        return self._gru_ctx[0], self._mlp_ctx[1], self._mlp_ctx[2]

    def backward(self, d_emb, relu_mask=None):
        """As OracleTGN.backward, + the MLP's gradients.  ``relu_mask`` bool[n_ids, hidden] (rows in the order of
        ``mlp_rows()``): differentiate the hidden layer with these ReLU decisions instead of the forward's own."""
        grads = {k: np.zeros_like(v) for k, v in self.P.items()}
        d_mem = np.zeros((self.n_nodes, self.D), self.dtype)
        self._embed_backward(self._ctx, np.asarray(d_emb, self.dtype), grads, d_mem)
        if self._gru_ctx is not None and self._gru_ctx[1] is not None:
            ids, cache = self._gru_ctx
            W_ih, W_hh, _, _ = self._gru()
            g = T.gru_cell_backward(cache, d_mem[ids], W_ih, W_hh, self.dtype)
            for k, v in g.items():
                grads[GRU + k] += v.astype(self.dtype)
            d_x, _ = gru_input_backward(cache, d_mem[ids], W_ih, self.dtype)
            gm, _ = mlp_backward(self._mlp_ctx, d_x, self._mlp()[2], relu_mask)
            for k, v in gm.items():
                grads[MLP + k] += v.astype(self.dtype)
        return grads


def f64_twin(ref):
    """parity.f64_twin for the MLP model (a shallow copy keeps the class)."""
    import parity
    return parity.f64_twin(ref)


def init_params(D, Ef, n_layers, msg_dim, seed=0):
    """oracle.init_params with the MLP's tensors and the narrower weight_ih."""
    P = T.init_params(D, Ef, n_layers, seed, use_memory=True)
    rs = np.random.RandomState(seed + 77)
    M = 3 * D + Ef

    def lin(o, i):
        return (rs.randn(o, i) * np.sqrt(1.0 / i)).astype(f32)
    P[GRU + "weight_ih"] = lin(3 * D, msg_dim)
    P[MLP + "0.weight"] = lin(M // 2, M); P[MLP + "0.bias"] = (rs.randn(M // 2) * 0.1).astype(f32)
    P[MLP + "2.weight"] = lin(msg_dim, M // 2); P[MLP + "2.bias"] = (rs.randn(msg_dim) * 0.1).astype(f32)
    return P


def load_golden_state(g, pre, ref):
    """The reference's state in front of recorded step ``pre`` of a g11 fixture, into the host model ``ref``."""
    from collections import defaultdict
    P = {}
    for k in g.files:
        if k.startswith(pre + "sd_"):
            name = k[len(pre + "sd_"):]
            if name in ("memory.memory", "memory.last_update") or "layer_norm" in name or name.startswith(ALIAS):
                continue
            P[name] = g[k].astype(ref.dtype)
    ref.P = P
    ref.memory = g[pre + "sd_memory.memory"].astype(ref.dtype)
    ref.last_update = g[pre + "sd_memory.last_update"].copy()
    ref.messages = defaultdict(list)
    tab, mt, cnt = g[pre + "msg_tab"], g[pre + "msg_t"], g[pre + "msg_cnt"]
    for nid in np.nonzero(cnt)[0]:
        ref.messages[int(nid)] = [(tab[nid].astype(ref.dtype), mt[nid])]
