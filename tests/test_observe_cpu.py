"""CPU side of ``TGN.observe``: the reference helper of its tests held to the reference's own goldens, the two new symbols
of the C ABI and their argument checks, and the host-side validation of the Python entry point."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
import observe_ref as O


# ---------------------------------------------------------------------------------------------- the helper against the goldens
@pytest.mark.parametrize("fixture", O.MEM_FIXTURES)
def test_reference_helper_reproduces_the_goldens_state_update(fixture):
    """For every recorded step the fixture's state in front of the step is injected and the batch observed: the tables must
    be the ones the reference itself left behind that step - which embedded the batch, and whose state update cannot
    depend on that.  No new golden, nothing from the reference tree."""
    g = load_golden(fixture)
    assert bool(g["use_memory"]) and tuple(int(s) for s in g["recorded_steps"]) == O.STEPS
    o = O.golden_oracle(g)
    for step in O.STEPS:
        pre = "s%d_" % step
        O.load_golden_state(o, g, pre)
        o.observe(g[pre + "src"], g[pre + "dst"], g[pre + "ts"], g[pre + "eidx"])
        e_mem, e_tab = O.check_tables(o.tables(), O.golden_after(g, pre), (fixture, step))
        print("FIGURES observe helper %s step %d: memory relerr %.3g, message relerr %.3g" % (fixture, step, e_mem, e_tab))


def test_reference_helper_batch_walk_is_the_serial_chain():
    w = O.random_world(3, 30, 8, 4, 50)
    rs = np.random.RandomState(0)
    src, dst = rs.randint(1, 30, 20), rs.randint(1, 30, 20)
    ts, eidx = 100.0 + np.arange(20.0), rs.randint(1, 51, 20)
    a, b = O.world_oracle(w), O.world_oracle(w)
    assert a.observe_log(src, dst, ts, eidx, batch_size=8) == 20
    for k in (0, 8, 16):
        b.observe(src[k:k + 8], dst[k:k + 8], ts[k:k + 8], eidx[k:k + 8])
    assert all(np.array_equal(x, y) for x, y in zip(a.tables(), b.tables()))
    c = O.world_oracle(w)
    c.observe_log(src, dst, ts, eidx)                          # one batch of 20: another function of the log
    assert not np.array_equal(c.tables()[2], a.tables()[2])


# ---------------------------------------------------------------------------------------------- the C ABI
def _cfg(use_memory=1, D=16):
    from pfotgnrec_amd import _lib
    return _lib.TgnConfig(141, 500, D, 4, 1, 2, use_memory, 1, 1, 1)


def test_abi_exports_the_observe_symbols():
    from pfotgnrec_amd import _lib
    lib = _lib.load()
    for name in ("pfo_tgn_observe", "pfo_tgn_observe_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    assert lib.pfo_abi_version() == 6
    cfg = _cfg()
    small, large = (lib.pfo_tgn_observe_workspace_bytes(ctypes.byref(cfg), B) for B in (24, 8200))
    assert 0 < small < large
    # beyond 16384 events per batch the message store needs its winner table (one int per node) on top of the rows
    below, above = (lib.pfo_tgn_observe_workspace_bytes(ctypes.byref(cfg), B) for B in (8192, 8193))
    assert above - below >= 141 * 4
    assert lib.pfo_tgn_observe_workspace_bytes(ctypes.byref(cfg), 0) == -1
    assert lib.pfo_tgn_observe_workspace_bytes(ctypes.byref(_cfg(use_memory=0)), 24) == -1


def test_abi_rejects_bad_arguments_with_a_message():
    from pfotgnrec_amd import _lib
    lib = _lib.load()
    st = _lib.TgnState()
    cfg = _cfg()
    need = lib.pfo_tgn_observe_workspace_bytes(ctypes.byref(cfg), 24)

    def call(c, N, B, nbytes):
        _lib.call("pfo_tgn_observe", ctypes.byref(c), ctypes.byref(st), None, None, None, None, N, B, None, nbytes, None)
    with pytest.raises(_lib.PfoError, match="without memory"):
        call(_cfg(use_memory=0), 48, 24, need)
    with pytest.raises(_lib.PfoError, match="B must be"):
        call(cfg, 48, 0, need)
    with pytest.raises(_lib.PfoError, match="N must not be negative"):
        call(cfg, -1, 24, need)
    with pytest.raises(_lib.PfoError, match="workspace too small"):
        call(cfg, 48, 24, need - 1)
    with pytest.raises(_lib.PfoError, match="multiple of 4"):
        call(_cfg(D=30), 48, 24, need)
    call(cfg, 0, 24, 0)                                        # N == 0: nothing is queued, nothing is looked at


# ---------------------------------------------------------------------------------------------- TGN.observe on the host
class _RecordingFinder:
    """A finder that lives on the host and records what ``append`` hands it."""
    uniform, seed, n_nodes = False, 0, 61

    def __init__(self):
        self.appended = []

    def append(self, sources, destinations, edge_idxs, timestamps):
        self.appended.append(tuple(np.asarray(a).copy() for a in (sources, destinations, edge_idxs, timestamps)))
        return self


def _host_model(use_memory, finder=None):
    import pfotgnrec_amd as P
    from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
    g = make_graph(SyntheticConfig("t", 50, 10, 400, 8, 1, 4, 2), with_prices=False)
    nf = finder if finder is not None else P.get_neighbor_finder(g.data, False)
    tgn = P.TGN(nf, g.node_features, g.edge_features, "cpu", n_layers=1, n_heads=2, use_memory=use_memory, memory_dimension=8,
                message_function="identity")
    return tgn, g.data


def test_observe_validates_its_inputs_on_the_host():
    from pfotgnrec_amd import _lib
    tgn, d = _host_model(True)
    s, t, ts, e = d.sources[:6], d.destinations[:6], d.timestamps[:6], d.edge_idxs[:6]
    with pytest.raises(ValueError, match="same length"):
        tgn.observe(s, t[:5], ts, e)
    with pytest.raises(ValueError, match="same length"):
        tgn.observe(s, t, ts, e[:2])
    for bad in (0, -3):
        with pytest.raises(ValueError, match="batch_size"):
            tgn.observe(s, t, ts, e, batch_size=bad)
    with pytest.raises(IndexError, match="sources"):
        tgn.observe(np.array([tgn.n_nodes]), t[:1], ts[:1], e[:1])
    with pytest.raises(IndexError, match="destinations"):
        tgn.observe(s[:1], np.array([-1]), ts[:1], e[:1])
    with pytest.raises(IndexError, match="edge_idxs"):
        tgn.observe(s[:1], t[:1], ts[:1], np.array([tgn.edge_raw_features.shape[0]]))     # the table is not grown
    step, version = tgn._step, tgn.memory._state_version
    with pytest.raises(_lib.PfoError):                         # a model on the host: no CPU path, like every compute method
        tgn.observe(s, t, ts, e)
    assert (tgn._step, tgn.memory._state_version) == (step, version) and not tgn.memory._any_msg


def test_observe_without_memory_only_appends():
    nf = _RecordingFinder()
    tgn, d = _host_model(False, nf)
    s, t, ts, e = d.sources[:6], d.destinations[:6], d.timestamps[:6], d.edge_idxs[:6]
    assert tgn.observe(s, t, ts, e, batch_size=4) == 6 and nf.appended == []          # append is off by default
    assert tgn.observe(s, t, ts, e, batch_size=4, append=True) == 6
    assert len(nf.appended) == 1
    for got, want in zip(nf.appended[0], (s, t, e, ts)):
        assert np.array_equal(got, want)
    assert tgn.observe(s[:0], t[:0], ts[:0], e[:0], append=True) == 0 and len(nf.appended) == 1
    assert tgn._step == 0
