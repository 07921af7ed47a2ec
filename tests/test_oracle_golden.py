"""Pin the oracle (oracle/*.py) against fixtures captured from the reference itself (tools/make_golden.py)."""
import numpy as np
import pytest

from conftest import load_golden
from oracle.neighbor_finder import OracleNeighborFinder, build_adjacency
from oracle.rand_edge_sampler import OracleRandEdgeSampler
from oracle import mv_select as mv


# ---------------------------------------------------------------- G1 sampler (bit-exact)
@pytest.mark.parametrize("K", [10, 3, 0])
def test_g1_most_recent(K):
    g = load_golden("g1_sampler")
    nf = OracleNeighborFinder(*build_adjacency(g["a_src"], g["a_dst"], g["a_eidx"], g["a_ts"]))
    nb, ei, et = nf.get_temporal_neighbor(g["a_q_nodes"], g["a_q_ts"], K)
    for got, key in ((nb, "nbr"), (ei, "eidx"), (et, "et")):
        ref = g["a_K%d_%s" % (K, key)]
        assert got.dtype == ref.dtype and got.shape == ref.shape
        assert np.array_equal(got, ref)


@pytest.mark.parametrize("K", [4, 20])
def test_g1_adversarial(K):
    g = load_golden("g1_sampler")
    nf = OracleNeighborFinder(*build_adjacency(g["b_src"], g["b_dst"], g["b_eidx"], g["b_ts"]))
    nb, ei, et = nf.get_temporal_neighbor(g["b_q_nodes"], g["b_q_ts"], K)
    assert np.array_equal(nb, g["b_K%d_nbr" % K])
    assert np.array_equal(ei, g["b_K%d_eidx" % K])
    assert np.array_equal(et, g["b_K%d_et" % K])


def test_g1_uniform_same_rng_stream():
    """Same numpy calls in the same order: seeding the global RNG reproduces the reference bit for bit."""
    g = load_golden("g1_sampler")
    nf = OracleNeighborFinder(*build_adjacency(g["b_src"], g["b_dst"], g["b_eidx"], g["b_ts"]), uniform=True)
    np.random.seed(int(g["b_uni_seed"]))
    log = []
    nb, ei, et = nf.get_temporal_neighbor(g["b_q_nodes"], g["b_q_ts"], 5, draw_log=log)
    assert np.array_equal(nb, g["b_uni_nbr"]) and np.array_equal(ei, g["b_uni_eidx"]) and np.array_equal(et, g["b_uni_et"])
    draws = g["b_uni_draws"]
    for i, _, idx in log:
        assert np.array_equal(idx, draws[i])


def test_g1_uniform_injected_draws_canonical_sort():
    """Injected draws + stable re-sort: equal to the reference up to permutations inside equal-time groups (App. A-9)."""
    g = load_golden("g1_sampler")
    nf = OracleNeighborFinder(*build_adjacency(g["b_src"], g["b_dst"], g["b_eidx"], g["b_ts"]), uniform=True)
    nb, ei, et = nf.gather_uniform(g["b_q_nodes"], g["b_q_ts"], g["b_uni_draws"], 5)
    assert np.array_equal(et, g["b_uni_et"])                      # times are sorted either way
    for i in range(len(nb)):
        for t in np.unique(et[i]):
            m = et[i] == t
            assert sorted(zip(nb[i][m], ei[i][m])) == sorted(zip(g["b_uni_nbr"][i][m], g["b_uni_eidx"][i][m]))


# ---------------------------------------------------------------- G10 sampler on yyyymmddHHMMSS timestamps
# Near 2.02e13 one f32 step is 2**21 (about two calendar days): the f32 edge times of utils.py:179-180 collapse ~35 distinct
# f64 times into one value, the deltas of embedding_module.py:133-135 (f64 query - f32 edge time) go negative where the edge
# time rounds up past the query, and the uniform re-sort (utils.py:201) meets ties between different edges on most rows.
def _g10_finder(g, uniform=False):
    return OracleNeighborFinder(*build_adjacency(g["src"], g["dst"], g["eidx"], g["ts"], int(g["q_nodes"].max())), uniform=uniform)


def _equal_up_to_tie_permutation(nb, ei, et, ref_nb, ref_ei):
    for i in range(len(nb)):
        for t in np.unique(et[i]):
            m = et[i] == t
            assert sorted(zip(nb[i][m], ei[i][m])) == sorted(zip(ref_nb[i][m], ref_ei[i][m])), i


@pytest.mark.parametrize("K", [10, 3])
def test_g10_most_recent_real_timestamps(K):
    g = load_golden("g10_realts_sampler")
    nb, ei, et = _g10_finder(g).get_temporal_neighbor(g["q_nodes"], g["q_ts"], K)
    for got, key in ((nb, "nbr"), (ei, "eidx"), (et, "et")):
        ref = g["K%d_%s" % (K, key)]
        assert got.dtype == ref.dtype and np.array_equal(got, ref), key
    dt = (g["q_ts"][:, None] - et).astype(np.float32)             # embedding_module.py:133-135
    assert np.array_equal(dt, g["K%d_dt" % K])
    if K == 10:
        assert int((dt < 0).sum()) == int(g["n_negative_dt"]) > 0


def test_g10_uniform_real_timestamps():
    """The reference's slot order inside an f32 tie group is its platform's (default argsort, utils.py:201); the canonical
    order is the stable one.  Times exact, (neighbour, edge) pairs equal up to permutation inside tie groups."""
    g = load_golden("g10_realts_sampler")
    nf = _g10_finder(g, uniform=True)
    nb, ei, et = nf.gather_uniform(g["q_nodes"], g["q_ts"], g["uni_draws"], 5)
    assert np.array_equal(et, g["uni_et"])
    _equal_up_to_tie_permutation(nb, ei, et, g["uni_nbr"], g["uni_eidx"])
    assert np.array_equal((g["q_ts"][:, None] - et).astype(np.float32), g["uni_dt"])
    ties = sum(any(et[i, a] == et[i, b] and ei[i, a] != ei[i, b] for a in range(5) for b in range(a)) for i in range(len(et)) if nb[i].any())
    assert ties == int(g["uni_n_tie_rows"]) > 0
    assert int(((ei != g["uni_eidx"]).any(1)).sum()) == int(g["uni_n_unstable_rows"])
    # same global RNG stream: the draws themselves are reproduced (the slot order of the outputs is not asserted)
    np.random.seed(int(g["uni_seed"]))
    log = []
    _, _, et2 = nf.get_temporal_neighbor(g["q_nodes"], g["q_ts"], 5, draw_log=log)
    assert np.array_equal(et2, g["uni_et"]) and len(log) == int((g["uni_draws"][:, 0] >= 0).sum())
    for i, _, idx in log:
        assert np.array_equal(idx, g["uni_draws"][i])


def test_gather_uniform_refuses_draws_outside_the_history():
    g = load_golden("g10_realts_sampler")
    nf = _g10_finder(g, uniform=True)
    draws = g["uni_draws"].copy()
    row = int(np.flatnonzero(draws[:, 0] >= 0)[3])
    draws[row, 2] = len(nf.find_before(int(g["q_nodes"][row]), g["q_ts"][row])[0])
    with pytest.raises(ValueError, match="row %d " % row):
        nf.gather_uniform(g["q_nodes"], g["q_ts"], draws, 5)
    draws[row, 2] = -1
    with pytest.raises(ValueError, match="row %d " % row):
        nf.gather_uniform(g["q_nodes"], g["q_ts"], draws, 5)


def test_g10_fixture_tells_an_f32_query_time_apart():
    """Wrong arithmetic restated: the query time cast to f32 in front of the search (utils.py:158 searches with the f64 time).
    The fixture's neighbours differ on many rows, so a kernel that narrows the query cannot pass the g10 comparisons."""
    g = load_golden("g10_realts_sampler")
    nf = _g10_finder(g)
    wrong_nb, wrong_ei, _ = nf.get_temporal_neighbor(g["q_nodes"], g["q_ts"].astype(np.float32), 10)
    rows = ((wrong_nb != g["K10_nbr"]) | (wrong_ei != g["K10_eidx"])).any(1)
    assert int(g["n_f32_query_rows"]) > 0 and rows.sum() > 0
    assert rows.sum() >= len(rows) // 10, rows.sum()            # not a corner: a tenth of the rows at least


def test_g10_fixture_tells_an_f32_delta_apart():
    """Wrong arithmetic restated: f32(t) - f32(t_e) instead of f64(t) - f32(t_e) (embedding_module.py:133-135)."""
    g = load_golden("g10_realts_sampler")
    for key in ("K10", "K3", "uni"):
        wrong = g["q_ts"].astype(np.float32)[:, None] - g[key + "_et"]
        assert wrong.dtype == np.float32
        differ = (wrong != g[key + "_dt"]) & (g[key + "_nbr"] != 0)
        assert differ.sum() >= differ.size // 10, (key, differ.sum())
    # the all-f32 difference is a multiple of the f32 step and never negative for an edge before t: the negative entries go too
    wrong = g["q_ts"].astype(np.float32)[:, None] - g["K10_et"]
    assert int(g["n_negative_dt"]) > 0 and not (wrong[g["K10_nbr"] != 0] < 0).any()
    assert int(g["n_same_step_rows"]) > 0 and int(g["n_rounded_past_rows"]) > 0


def test_g10_day_key_of_every_interaction():
    """main.py:212 ``str(ts)[:8]``: the host-side day lookup (the pickle ingest + ``day_indices``, and the evaluation tables'
    ``day_indices``) returns the reference's day for every interaction of the g10 graph."""
    from pfotgnrec_amd.mv_sampler import prices_from_time_feature, day_indices
    from pfotgnrec_amd.evaluation import InvestTables
    g = load_golden("g10_realts_sampler")
    keys = [str(k) for k in g["day_keys"]]
    assert len(set(k[:4] for k in keys)) == 2 and all(len(k) == 8 for k in keys)       # both years of the boundary
    codes = ["%06d" % (i + 1) for i in range(3)]
    map_item_id = {c: i for i, c in enumerate(codes)}
    time_feature = {k: {c: np.full(30, 100.0 + j) for j, c in enumerate(codes)} for k in sorted(set(keys), reverse=True)}
    days, arr = prices_from_time_feature(time_feature, map_item_id)
    assert days == sorted(set(keys)) and arr.shape == (len(days), 3, 30)
    idx = day_indices(g["ts"], days)
    assert [days[i] for i in idx] == keys
    tables = InvestTables.from_prices(days, arr, arr, map_item_id)
    assert np.array_equal(tables.day_indices(g["ts"]), idx)
    assert np.array_equal(day_indices(g["ts"].astype(np.int64), days), idx)             # integer timestamps name the same day
    with pytest.raises(KeyError):
        day_indices([g["ts"][0] + 1e8], days)                                           # a month the tables do not list


# ---------------------------------------------------------------- G2 candidate draw
def _portfolios(g, codes):
    return [[codes[j] for j in row[:n]] if n > 0 else [""] for row, n in zip(g["port_idx"], g["port_len"])]


@pytest.mark.parametrize("size", [3, 20, 30])
def test_g2_candidates(size):
    g = load_golden("g2_candidates")
    n_items, upper_u = int(g["n_items"]), int(g["upper_u"])
    codes = ["%06d" % (i + 1) for i in range(n_items)]
    map_item_id = {c: i for i, c in enumerate(codes)}
    seed = int(g["seed_size%d" % size])
    np.random.seed(5)
    avail = []
    s = OracleRandEdgeSampler(g["src"], g["dst_all"], _portfolios(g, codes), upper_u, map_item_id, seed=None if seed < 0 else seed)
    neg = s.sample(size, available_log=avail)
    ref = g["neg_size%d" % size]
    assert np.array_equal(neg, ref)                               # same RNG stream, same calls
    for b in range(len(ref)):                                      # semantics the device draw must keep (App. A-8)
        assert set(ref[b]) <= set(avail[b])
        port = set(g["port_idx"][b][:g["port_len"][b]] + upper_u + 1)
        assert not (set(ref[b]) & port)
        if len(avail[b]) >= size:
            assert len(set(ref[b])) == size


# ---------------------------------------------------------------- G3 MV selection
@pytest.mark.parametrize("lam", [0.5, 0.1])
def test_g3_mv(lam):
    g = load_golden("g3_mv")
    pre = "lam%02d_" % int(lam * 10)
    upper_u = int(g["upper_u"])
    neg = g[pre + "neg"]
    cand = np.concatenate([g["dst"][:, None], neg], 1) - (upper_u + 1)
    p_pos, p_neg, Y, NR = mv.mv_select(g["prices"], g[pre + "day_idx"], cand, g["port_idx"], g["port_len"],
                                       float(g["gamma"]), lam, 1, 3, platform_order=True)
    assert np.array_equal(Y, g[pre + "y_mv"])                      # same numpy calls -> bit-exact fp64
    assert np.array_equal(NR, g[pre + "new_rank"])
    assert np.array_equal(p_pos.flatten() + upper_u + 1, g[pre + "p_pos"])
    assert np.array_equal(p_neg.flatten() + upper_u + 1, g[pre + "p_neg"])
    # canonical tie policy: identical wherever the selection is tie-free, a valid tie permutation elsewhere
    cp, cn, _, _ = mv.mv_select(g["prices"], g[pre + "day_idx"], cand, g["port_idx"], g["port_len"], float(g["gamma"]), lam, 1, 3)
    n_tiefree = 0
    for b in range(len(cand)):
        nr = NR[b]
        order_ref = g[pre + "order"][b]
        order_can = mv.canonical_order(nr)
        assert np.array_equal(nr[order_ref], nr[order_can])        # same rank sequence
        uniq = len(np.unique(nr)) == len(nr)
        if uniq:
            n_tiefree += 1
            assert np.array_equal(cp[b], p_pos[b]) and np.array_equal(cn[b], p_neg[b])
    assert n_tiefree >= 0


def test_g3_both_branches_present():
    g = load_golden("g3_mv")
    assert (g["port_len"] == 0).any() and (g["port_len"] > 0).any()
