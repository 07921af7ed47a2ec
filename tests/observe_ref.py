"""CPU reference of ``TGN.observe`` and the helpers its CPU and GPU tests share.

``ObserveOracle`` restates the state half of the oracle's ``_step`` (oracle/tgn_oracle.py, the lines behind ``_embed``:
``_update_memory(positives)``, clear, two ``_get_raw_messages``) and nothing else - no ``_embed``.  It is itself pinned by
the reference's goldens (tests/test_observe_cpu.py).  Importable without a GPU."""
from collections import defaultdict

import numpy as np

from oracle import tgn_oracle as T
from parity import relerr

RTOL = 1e-4          # the project's bar for state tables: max |a - b| / max |b|

# every golden fixture with memory, and the steps they record
MEM_FIXTURES = ["g5_step_L1_mem", "g5_step_L2_mem", "g5_step_L1_mem_p", "g10_realts_step_L1_mem", "g10_realts_step_L2_mem",
                "g10_realts_step_L1_mem_p"]
STEPS = (2, 3, 4)


class ObserveOracle(T.OracleTGN):
    def observe(self, src, dst, ts, eidx):
        """One batch: tgn.py:295-317 without the embedding in front of it."""
        src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
        positives = np.concatenate([src, dst])
        self._update_memory(positives)                                          # tgn.py:295
        for nid in positives:                                                   # tgn.py:302
            self.messages[int(nid)] = []
        self._get_raw_messages(src, dst, ts, eidx)                              # tgn.py:304-317
        self._get_raw_messages(dst, src, ts, eidx)

    def observe_log(self, src, dst, ts, eidx, batch_size=None):
        n = len(src)
        b = n if batch_size is None else int(batch_size)
        for k in range(0, n, max(b, 1)):
            self.observe(src[k:k + b], dst[k:k + b], ts[k:k + b], eidx[k:k + b])
        return n

    def tables(self):
        """(memory, last_update, msg_table, msg_time, has_msg) in the device layout."""
        tab, t, has = self.pending_table()
        return self.memory, self.last_update, tab, t, has


def golden_oracle(g):
    return ObserveOracle(None, g["node_features"], g["edge_features"], {}, int(g["L"]), int(g["H"]), use_memory=True)


def load_golden_state(o, g, pre):
    """Parameters, memory, last_update and pending messages the fixture stores in front of step ``pre``."""
    P = {}
    for k in g.files:
        if k.startswith(pre + "sd_"):
            name = k[len(pre + "sd_"):]
            if name in ("memory.memory", "memory.last_update") or "layer_norm" in name:
                continue
            P[name] = g[k].astype(np.float32)
    o.P = P
    o.memory = g[pre + "sd_memory.memory"].copy()
    o.last_update = g[pre + "sd_memory.last_update"].copy()
    o.messages = defaultdict(list)
    tab, mt, cnt = g[pre + "msg_tab"], g[pre + "msg_t"], g[pre + "msg_cnt"]
    for nid in np.nonzero(cnt)[0]:
        o.messages[int(nid)] = [(tab[nid], mt[nid])]


def check_tables(got, want, tag=""):
    """``got`` / ``want`` = (memory, last_update, msg_table, msg_time, has_msg): the has-message pattern, last_update and the
    message times exact, memory and message rows within the bar.  Returns the two measured errors."""
    mem, lu, tab, mt, has = (np.asarray(a) for a in got)
    wmem, wlu, wtab, wmt, whas = (np.asarray(a) for a in want)
    whas = whas > 0
    assert np.array_equal(has > 0, whas), (tag, "has_msg")
    assert np.array_equal(lu.view(np.int32), wlu.astype(np.float32).view(np.int32)), (tag, "last_update")
    assert np.array_equal(mt[whas].view(np.int32), wmt.astype(np.float32)[whas].view(np.int32)), (tag, "msg_time")
    e_mem = relerr(mem, wmem)
    e_tab = relerr(tab[whas], wtab[whas]) if whas.any() else 0.0
    assert e_mem < RTOL, (tag, "memory", e_mem)
    assert e_tab < RTOL, (tag, "msg_table", e_tab)
    return e_mem, e_tab


def golden_after(g, pre):
    return (g[pre + "after_memory"], g[pre + "after_last_update"], g[pre + "after_msg_tab"], g[pre + "after_msg_t"],
            g[pre + "after_msg_cnt"] > 0)


# ---------------------------------------------------------------------------- hand-made worlds (random parameters and state)
def random_world(seed, n_nodes, D, Ef, n_edges, pending=0.5, L=1, H=2):
    """Random features, parameters and model state on ``n_nodes`` nodes (node 0 = padding): memory rows ~ N(0, 0.5),
    last_update in [0, 50), a pending message on about ``pending`` of the nodes 1.. at a time in [last_update, 100)."""
    rs = np.random.RandomState(seed)
    M = 3 * D + Ef
    w = dict(n_nodes=n_nodes, D=D, Ef=Ef, L=L, H=H,
             node_features=rs.randn(n_nodes, D).astype(np.float32),
             edge_features=rs.randn(n_edges + 1, Ef).astype(np.float32),
             params=T.init_params(D, Ef, L, seed=seed + 1))
    mem = (rs.randn(n_nodes, D) * 0.5).astype(np.float32)
    lu = np.floor(rs.rand(n_nodes) * 50).astype(np.float32)
    has = rs.rand(n_nodes) < pending
    has[0] = False
    tab = (rs.randn(n_nodes, M) * 0.5).astype(np.float32) * has[:, None]
    mt = np.where(has, lu + np.floor(rs.rand(n_nodes) * 50), 0).astype(np.float32)
    w["state"] = (mem, lu, tab, mt, has)
    return w


def world_oracle(w, state=True):
    o = ObserveOracle(None, w["node_features"], w["edge_features"], w["params"], w["L"], w["H"], use_memory=True)
    if state:
        mem, lu, tab, mt, has = w["state"]
        o.memory, o.last_update = mem.copy(), lu.copy()
        for nid in np.nonzero(has)[0]:
            o.messages[int(nid)] = [(tab[nid].copy(), mt[nid])]
    return o
