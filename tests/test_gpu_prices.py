"""GPU tests of the price ledger: ``pfo_returns_append_day`` / ``pfo_returns_scatter_closes`` / ``pfo_day_lookup`` on
raw tensors with canaries around what they may write, ``PriceLedger`` against the numpy rules of ``prices_ref`` (ring, shift,
carry-forward, growth, expiry, persistence, lookup) and ``TGN.recommend(mv=ledger)`` against ``mv=MVSampler`` and against the
ledger's own table fed through the duck-typed route.  Every comparison is bitwise except one: the newest return of a day is a
logarithm, and two faithful libms need not agree in the last place - its quotient is compared bitwise, its value is held to
the long-double logarithm within ``BAR`` ulps (``_bar``: numpy's own measured distance from that reference plus one)."""
import types

import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

import pfotgnrec_amd as P
from pfotgnrec_amd.mv_sampler import day_indices
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
import prices_ref as PR

DEV = "cuda:0"
CANARY = -7.5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---------------------------------------------------------------------------------------------- the one float comparison
def _ulps(got, ref):
    """Distance of ``got`` from ``ref`` in ulps of ref (both f64; where ref is 0 got must be 0)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    zero = ref == 0
    d = np.abs(got - ref) / np.spacing(np.abs(np.where(zero, 1.0, ref)))
    return np.where(zero, np.where(got == 0, 0.0, np.inf), d)


def _log_ref(q):
    assert np.finfo(np.longdouble).nmant >= 63, "the reference logarithm needs a long double wider than fp64"
    return np.log(np.asarray(q, np.float64).astype(np.longdouble)).astype(np.float64)


_QUOT = {}


def _quotients():
    """(last_close, close, quotient) for 3 x 2^18 price steps: lognormal daily steps, 1 +- 1e-3, U(0.5, 2) - computed once."""
    if not _QUOT:
        rs = np.random.RandomState(11)
        n = 1 << 18
        last = rs.uniform(1.0, 1000.0, size=3 * n)
        step = np.concatenate([np.exp(rs.randn(n) * 0.02), 1.0 + rs.uniform(-1e-3, 1e-3, size=n), rs.uniform(0.5, 2.0, size=n)])
        close = last * step
        q = close / last                                         # the fp64 quotient, on the host
        ref = _log_ref(q)
        _QUOT.update(last=last, close=close, q=q, ref=ref, numpy_max=float(_ulps(np.log(q), ref).max()))
    return _QUOT


def _bar():
    """numpy's measured maximum distance from the long-double logarithm, plus one ulp: not derived from the kernel."""
    return _quotients()["numpy_max"] + 1.0


def _check_newest(got, quot, what=""):
    """The newest returns ``got`` of the stocks with a quotient lie within the bar; the others are +0 bits."""
    has = ~np.isnan(quot)
    assert PR.same_bits(got[~has], np.zeros((~has).sum())), "%s: +0 where no logarithm was taken" % what
    if has.any():
        d = _ulps(got[has], _log_ref(quot[has]))
        assert d.max() <= _bar(), "%s: %.3g ulps from the reference, the bar is %.3g" % (what, d.max(), _bar())
    one = quot == 1.0
    assert PR.same_bits(got[one], np.zeros(one.sum())), "%s: a quotient of exactly 1.0 gives +0" % what


def test_newest_return_against_the_long_double_logarithm():
    """Measured on the MI355X: the kernel's maximum distance is 1 ulp from the rounded long-double logarithm (numpy's: 1 ulp),
    the bar is numpy's maximum plus one = 2."""
    Q = _quotients()
    n = Q["q"].shape[0]
    returns = torch.zeros((2, n, 2), dtype=torch.float64, device=DEV)
    keys = torch.zeros(2, dtype=torch.int64, device=DEV)
    last = _dev(Q["last"])
    quot = P.returns_append_day(returns, keys, last, 0, 1, n, 5, _dev(Q["close"]), want_quotients=True)
    assert PR.same_bits(_host(quot), Q["q"]), "the kernel's quotient is the host's fp64 quotient, bit for bit"
    got = _host(returns)[1, :, 1]
    d = _ulps(got, Q["ref"])
    differ = float((got != Q["ref"]).mean())
    print("FIGURES newest return vs long double log over %d quotients: kernel max %.3g ulps (differs on %.3g %%), numpy max %.3g ulps "
          "(differs on %.3g %%)" % (n, d.max(), 100 * differ, Q["numpy_max"], 100 * float((np.log(Q["q"]) != Q["ref"]).mean())))
    assert Q["numpy_max"] <= 1.0, "numpy's own logarithm is faithful here"
    assert d.max() <= _bar()
    assert PR.same_bits(_host(last), Q["close"]) and _host(keys).tolist() == [0, 5]
    assert not _host(returns)[0].any() and not _host(returns)[1, :, 0].any()


# ---------------------------------------------------------------------------------------------- 1. append on raw tensors
def _weird(rs, shape):
    """Doubles of every kind: the shifted part must be copied, not computed."""
    a = rs.randn(*shape)
    flat = a.reshape(-1)
    pick = rs.rand(flat.size)
    flat[pick < 0.05] = -0.0
    flat[(pick >= 0.05) & (pick < 0.1)] = np.inf
    bits = flat.view(np.int64)
    nan = (pick >= 0.1) & (pick < 0.15)
    bits[nan] = 0x7FF0000000000000 | rs.randint(1, 1 << 30, size=int(nan.sum()))      # NaNs with payloads, quiet and signalling
    bits[(pick >= 0.15) & (pick < 0.2)] = rs.randint(1, 1 << 20, size=int(((pick >= 0.15) & (pick < 0.2)).sum()))   # subnormals
    return a


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_append_on_raw_tensors_with_canaries(n):
    rs = np.random.RandomState(n)
    cap, pad = 3, 3
    for n_ret in (2, 29, 128):
        for form in ("dense", "dense_short", "sparse", "first_day"):
            table = np.full((cap, n + pad, n_ret), CANARY)
            table[0, :n] = _weird(rs, (n, n_ret))
            keys = np.array([11, -99, -99], np.int64)
            last = np.full(n + pad, CANARY)
            last[:n] = rs.uniform(1.0, 100.0, size=n)
            last[:n][rs.rand(n) < 0.2] = np.nan                  # never quoted so far
            closes = last[:n] * np.exp(rs.randn(n) * 0.05)
            closes[np.isnan(closes)] = 50.0                      # first quotes
            closes[rs.rand(n) < 0.2] = np.nan                    # not quoted today
            same = rs.rand(n) < 0.2
            closes[same] = last[:n][same]                        # a quotient of exactly 1.0 (NaN where never quoted: not quoted)
            bad = rs.rand(n) < 0.15
            closes[bad] = np.array([0.0, -4.0, np.inf, -np.inf])[rs.randint(0, 4, size=int(bad.sum()))]     # skipped by the kernel
            prev, new = (-1, 2) if form == "first_day" else (0, 2)
            d_tab, d_keys, d_last = _dev(table), _dev(keys), _dev(last)
            if form == "sparse":
                # every stock twice at shuffled positions (the later valid one wins), indices outside the table, a stale stamp table
                pos = np.concatenate([rs.permutation(n), rs.permutation(n)])
                vals = np.concatenate([np.where(rs.rand(n) < 0.5, rs.uniform(1.0, 100.0, size=n), np.nan), closes[pos[n:]]])
                pos = np.concatenate([pos, [-1, n, n + 2, 2 ** 31 - 1]]).astype(np.int32)
                vals = np.concatenate([vals, [5.0] * 4])
                order = rs.permutation(len(pos))
                pos, vals = pos[order], vals[order]
                stamp = torch.full((n + 1,), 2 ** 31 - 1, dtype=torch.int32, device=DEV)
                stamp = P.returns_scatter_closes(_dev(pos), _dev(vals), n, stamp)
                assert int(stamp[n]) == 2 ** 31 - 1, "the stamp table is written up to n_stocks alone"
                today = np.full(n, np.nan)
                for p in range(len(pos)):
                    if 0 <= pos[p] < n and PR.close_ok(vals[p]):
                        today[pos[p]] = vals[p]
                quot = P.returns_append_day(d_tab, d_keys, d_last, prev, new, n, 12, _dev(vals), stamp, want_quotients=True)
            else:
                given = closes[:n // 2] if form == "dense_short" else closes
                today = np.full(n, np.nan)
                today[:len(given)] = np.where(np.isfinite(given) & (given > 0), given, np.nan)
                quot = P.returns_append_day(d_tab, d_keys, d_last, prev, new, n, 12, _dev(given), want_quotients=True)
            got, got_keys, got_last, quot = _host(d_tab), _host(d_keys), _host(d_last), _host(quot)
            what = "n=%d n_ret=%d %s" % (n, n_ret, form)
            quoted = ~np.isnan(today)
            want_q = np.where(quoted & ~np.isnan(last[:n]), today / last[:n], np.nan)
            assert PR.same_bits(quot, want_q), what + ": quotients"
            shifted = np.zeros((n, n_ret - 1)) if form == "first_day" else table[0, :n, 1:]
            assert PR.same_bits(got[2, :n, :-1], shifted), what + ": the shifted part is the previous day's, bitwise"
            _check_newest(got[2, :n, -1], want_q, what)
            assert PR.same_bits(got[:2], table[:2]) and PR.same_bits(got[2, n:], table[2, n:]), what + ": canaries behind the live rows"
            assert got_keys.tolist() == [11, -99, 12]
            assert PR.same_bits(got_last[:n], np.where(quoted, today, last[:n])) and PR.same_bits(got_last[n:], last[n:]), what + ": carry-forward"
            if n >= 63:
                assert (want_q == 1.0).any() or form != "dense"
                assert quoted.any() and (~quoted).any() and np.isnan(last[:n]).any()


# ---------------------------------------------------------------------------------------------- 2. the ledger against the reference
def _same_ledger(led, ref, what=""):
    st, want = led.state(), ref.state()
    assert (led.head, led.n_days, led.n_stocks, led.day_cap) == (ref.head, ref.n_days, ref.n_stocks, ref.day_cap), what
    for k in ("day_keys", "returns", "last_close"):
        assert PR.same_bits(st[k], want[k]), "%s: %s" % (what, k)
    full = _host(led.returns)
    assert not full[:, led.n_stocks:].any(), what + ": rows behind the live stock count are zeros"
    assert PR.same_bits(_host(led.day_keys)[ref.slots()], want["day_keys"])


def _tick(led, ref, key, closes, stocks=None, on_dev=False, what=""):
    """One day into both; the reference takes the device's logarithms after they were held to the bar."""
    grow = not (on_dev and stocks is not None)
    if on_dev:
        led.append_day(key, _dev(np.asarray(closes, np.float64)), None if stocks is None else _dev(np.asarray(stocks, np.int32)))
    else:
        led.append_day(key, closes, stocks)
    newest = _host(led.returns)[(led.head + led.n_days - 1) % led.day_cap, :led.n_stocks, -1]
    before = ref.last_close.copy()
    quot = ref.append_day(key, closes, stocks, grow=grow, newest=newest)
    _check_newest(newest, quot, what)
    _same_ledger(led, ref, what)
    return quot, before


@pytest.mark.parametrize("n_ret", [2, 29])
def test_ledger_appends_like_the_reference(n_ret):
    """Eleven days through the four routes; the stock axis grows by a longer dense array (host, then device) and by a sparse
    index; stock 300 is listed on day 6, first quoted on day 8 (+0) and moves from day 9 on."""
    rs = np.random.RandomState(n_ret)
    led, ref = P.PriceLedger(n_ret, 100, DEV), PR.RefLedger(n_ret)
    price = rs.uniform(10.0, 100.0, size=301)
    n_of_day = [5, 5, 5, 5, 70, 300, 301, 301, 301, 301, 301]
    routes = ["dense_host", "sparse_host", "dense_dev", "sparse_dev"]
    ptrs = set()
    for d, n in enumerate(n_of_day):
        route = routes[d % 4]
        price[:n] *= np.exp(rs.randn(n) * 0.03)
        quoted = rs.rand(n) < 0.7
        quoted[n - 1] = True                                      # (the sparse host form grows the table by its largest index)
        if n == 301:
            quoted[300] = d >= 8
        today = price[:n].copy()
        if d == 8:
            known = ~np.isnan(ref.last_close)
            today[:n:3] = np.where(known[:n:3], ref.last_close[:n:3], today[:n:3])     # quotients of exactly 1.0
            quoted[:n:3] = True
        if route.startswith("dense"):
            closes, stocks = np.where(quoted, today, np.nan), None
            if route == "dense_dev":
                closes[:n - 1][rs.rand(n - 1) < 0.1] = -1.0       # device inputs are not checked: skipped
                closes[0] = np.inf
        else:
            stocks = np.flatnonzero(quoted)[::-1].copy()
            closes = today[stocks]
            if route == "sparse_dev":
                # repeats: the last valid position wins; indices outside the table and bad closes: skipped
                stocks = np.concatenate([stocks, stocks[:3], [-2, led.n_stocks, 2 ** 31 - 1]])
                closes = np.concatenate([closes, closes[:3] * 1.5, [9.0, 9.0, 9.0]])
                closes[1], closes[-4] = 0.0, np.nan
        quot, _ = _tick(led, ref, 20240100 + d, closes, stocks, route.endswith("dev"), "day %d %s" % (d, route))
        assert led.n_stocks == n
        ptrs.add(led.returns.data_ptr())
        if d == 0:
            assert not ref.table.any(), "the first day is all zeros"
        if d == 8:
            assert (quot == 1.0).sum() > 50
    assert ref.n_days == 11 and ref.day_cap == 16 and len(ptrs) >= 5, "both axes grew, more than once"
    tab = ref.table
    assert not tab[:9, 300].any() and tab[9:, 300, -1].any(), "a stock first quoted mid-history starts at +0, then moves"
    assert (tab[:, :, -1] != 0).sum() > 500
    if n_ret == 29:
        assert (tab[10, :5, -10:] != 0).any() and not tab[10, :, :n_ret - 10].any(), "eleven days fill the newest ten columns"


@pytest.mark.parametrize("max_days", [1, 2, 3])
def test_ring_retention_expiry_reserve_and_state(max_days):
    rs = np.random.RandomState(max_days)
    n_ret, n = 4, 65
    led, ref = P.PriceLedger(n_ret, 100, DEV, max_days=max_days), PR.RefLedger(n_ret, max_days=max_days)
    full = PR.RefLedger(n_ret)                                   # the same days without retention
    price = rs.uniform(10.0, 100.0, size=n)
    for d in range(7):
        price = price * np.exp(rs.randn(n) * 0.03)
        closes = np.where(rs.rand(n) < 0.8, price, np.nan)
        survivors = led.state()
        _tick(led, ref, 10 * d, closes, None, d % 2 == 1, "max_days=%d day %d" % (max_days, d))
        full.append_day(10 * d, closes, newest=ref.table[-1, :, -1])
        assert led.n_days == min(d + 1, max_days) and led.keys == [10 * i for i in range(max(0, d + 1 - max_days), d + 1)]
        if max_days > 1 and d >= max_days:
            assert PR.same_bits(led.state()["returns"][:-1], survivors["returns"][1:]), "the survivors keep their bits"
        assert PR.same_bits(ref.table, full.table[-ref.n_days:]), "the window reaches through days that have left"
    assert led.day_cap == max(2, max_days) and (max_days == 1 or led.head != 0), "the ring has wrapped"
    # state -> load_state -> state
    st = led.state()
    other = P.PriceLedger(n_ret, 100, DEV, max_days=max_days)
    other.load_state(st)
    assert all(PR.same_bits(st[k], other.state()[k]) for k in st)
    # reserve on the wrapped ring: live rows bit for bit, then appends go on in the new layout
    led.reserve(n_days=5, n_stocks=80)
    ref.reserve_days(5)
    assert led.stock_cap == 80 and led.head == 0
    _same_ledger(led, ref, "reserve on a wrapped ring")
    with pytest.raises(ValueError):
        led.reserve(n_stocks=64)
    _tick(led, ref, 100, price * 1.01, None, True, "after reserve")
    _tick(other, PR.RefLedger.from_table(st["day_keys"], st["returns"], st["last_close"], max_days), 100, price * 1.01, None, False, "loaded")
    assert PR.same_bits(other.state()["returns"], led.state()["returns"])
    # expire_days before, inside and past the live range
    lo = led.keys[0]
    for before_key, gone in ((lo, 0), (lo - 5, 0), (led.keys[-1], led.n_days - 1), (10 ** 6, 1)):
        bits = _host(led.returns).tobytes()
        assert led.expire_days(before_key) == ref.expire_days(before_key) == gone
        assert _host(led.returns).tobytes() == bits, "no data moves"
        _same_ledger(led, ref, "expire_days(%d)" % before_key)
    assert led.n_days == 0
    _tick(led, ref, 10 ** 6 + 1, price, None, False, "a day after everything expired")
    assert led.state()["returns"][0, :, -1].any(), "the closes were carried through the expiry"


# ---------------------------------------------------------------------------------------------- 3. lookup
def _calendar_ledger():
    """A wrapped ring of calendar days with gaps: 9 trading days into max_days = 6, then the oldest (20240102) expired -> 5 live."""
    days = [20231227, 20231228, 20231229, 20240102, 20240103, 20240104, 20240105, 20240108, 20240109]
    led, ref = P.PriceLedger(2, 100, DEV, max_days=6), PR.RefLedger(2, max_days=6)
    for i, k in enumerate(days):
        led.append_day(k, np.array([10.0 + i]))
        ref.append_day(k, np.array([10.0 + i]))
    assert led.expire_days(20240103) == ref.expire_days(20240103) == 1
    assert led.head == ref.head == 4 and led.keys == days[4:] and led.day_cap == 6
    return led, ref, days


@pytest.mark.parametrize("U", [1, 63, 64, 65, 5000])
def test_day_lookup(U):
    led, ref, days = _calendar_ledger()
    rs = np.random.RandomState(U)
    # live days, days before the first, after the last, in the weekend gap, just expired (20240102) and pushed out by max_days
    pool = np.array(days[4:] + [20231226, 19991231, 20240110, 99991231, 20240106, 20240107, 20240102, 20231229, 20231228], np.int64)
    ymd = pool[np.arange(U) % len(pool)] if U > 1 else pool[:1]
    hms = np.array([0, 235959, 999999, 93000])[rs.randint(0, 4, size=U)]
    ts = (rs.permutation(ymd) * 1000000 + hms).astype(np.float64)
    got = _host(led.lookup(_dev(ts)))
    want = ref.lookup(ts)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    held = want >= 0
    assert held.any() and (U < 63 or ((~held).sum() > U // 3 and len(set(want[held].tolist())) == 5))
    # against day_indices on the 14-digit timestamps: ordinals among the live days, turned into slots
    assert np.array_equal(got[held], led.slots_of(day_indices(ts[held].astype(np.int64), led.keys)))
    assert np.array_equal(led.day_of(ts[held]), day_indices(ts[held].astype(np.int64), led.keys))
    for t in ts[~held][:3]:
        with pytest.raises(KeyError):
            day_indices(np.array([t]).astype(np.int64), led.keys)
        with pytest.raises(KeyError):
            led.day_of(np.array([t]))
    if U == 65:
        odd = np.array([np.nan, np.inf, -np.inf, -1.0, 1e300, 20240105000000.5])
        assert _host(led.lookup(_dev(odd))).tolist() == [-1, -1, -1, -1, -1, int(ref.lookup([20240105000000.0])[0])]
        empty = P.PriceLedger(2, 100, DEV)
        assert _host(empty.lookup(_dev(ts))).tolist() == [-1] * U
        assert tuple(led.lookup(_dev(ts[:0])).shape) == (0,)


# ---------------------------------------------------------------------------------------------- 4. end to end on the small world
N_USERS, N_ITEMS, K_NBR, CUT, WIDTH, N_DAYS = 120, 30, 5, 900, 8, 64
ITEMS = np.arange(N_USERS + 1, N_USERS + N_ITEMS + 1)
DIV = float(1 << 18)          # synthetic.day_of is floor(ts * 64 / 2^24): the key rule with this divisor


def _world():
    torch.manual_seed(6)
    g = make_graph(SyntheticConfig("t", N_USERS, N_ITEMS, 1500, 16, 1, K_NBR, 2), with_prices=True)
    d = g.data
    nf = P.NeighborFinder.from_arrays(d.sources[:CUT], d.destinations[:CUT], d.edge_idxs[:CUT], d.timestamps[:CUT], uniform=False,
                                      max_node_idx=g.node_features.shape[0] - 1)
    tgn = P.TGN(nf, g.node_features, g.edge_features[:CUT + 1], DEV, n_layers=1, n_heads=2, dropout=0.0, use_memory=True,
                memory_dimension=16, message_function="identity", n_neighbors=K_NBR)
    tgn.eval()
    tgn.track_holdings(WIDTH, g.upper_u)
    tgn.update_holdings(d.sources[:CUT], (g.portfolio_idx[:CUT], g.portfolio_len[:CUT]), d.timestamps[:CUT])
    assert g.prices.shape[0] == N_DAYS
    return g, tgn


def _model_state(t):
    m = t.memory
    tens = [t.flat_parameters, m.memory, m.last_update, m.msg_table, m.msg_time, m.has_msg, t.holdings.idx, t.holdings.len, t.holdings.time]
    return [x.detach().clone() for x in tens], (t.training, t._step, t._gru_applied_now, m._any_msg, m._state_version, t.n_nodes)


def _unchanged(t, before):
    now = _model_state(t)
    return now[1] == before[1] and all(torch.equal(a, b) for a, b in zip(now[0], before[0]))


def _queries(g, tgn):
    d = g.data
    users = np.unique(d.sources[:CUT])[:21]
    users = np.concatenate([users, users[:2]])
    ts = d.timestamps[CUT:CUT + 600:200][np.arange(len(users)) % 3]                  # three distinct times
    assert len(set(g.day_of(ts).tolist())) >= 2
    rows = tgn.holdings.rows(users)
    return users, ts, (rows[0].cpu().numpy(), rows[1].cpu().numpy())


FORMS = (("mv", dict()), ("basket", dict(basket=True)), ("held", dict(portfolios="held", exclude="held")))


def test_seeded_ledger_answers_like_the_mv_sampler():
    g, tgn = _world()
    users, ts, rows = _queries(g, tgn)
    mv = P.MVSampler(g.prices, g.upper_u, DEV, day_of=g.day_of)
    led = P.PriceLedger.from_prices(np.arange(N_DAYS), g.prices, g.upper_u, DEV, key_divisor=DIV)
    assert PR.same_bits(_host(led.returns), _host(mv.returns))
    assert np.array_equal(led.day_of(ts), g.day_of(ts))
    before = _model_state(tgn)
    n_moved = 0
    for name, kw in FORMS:
        kw = dict(dict(portfolios=rows), **kw)
        want = tgn.recommend(users, ts, 5, ITEMS, mv=mv, **kw)
        plain = tgn.recommend(users, ts, 5, ITEMS)
        n_moved += int(not torch.equal(want[0], plain[0]))
        for route, t_arg, day in (("host timestamps", ts, None), ("device timestamps", _dev(ts), None),
                                  ("explicit day_idx", ts, g.day_of(ts)), ("explicit device day_idx", _dev(ts), _dev(g.day_of(ts).astype(np.int32)))):
            got = tgn.recommend(users, t_arg, 5, ITEMS, mv=led, day_idx=day, **kw)
            assert len(got) == 4 and all(torch.equal(a, b) for a, b in zip(got, want)), "%s, %s" % (name, route)
        # a scalar time, on the host and on the device
        want = tgn.recommend(users, float(ts[0]), 5, ITEMS, mv=mv, **kw)
        for t_arg in (float(ts[0]), torch.tensor(float(ts[0]), dtype=torch.float64, device=DEV)):
            got = tgn.recommend(users, t_arg, 5, ITEMS, mv=led, **kw)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), "%s, scalar time" % name
    assert n_moved == 3, "the mean-variance side must move something, or the test shows nothing"
    assert _unchanged(tgn, before), "a query writes no model state"
    # a day the ledger does not hold: KeyError from host timestamps, an empty answer from device timestamps
    far = ts.copy()
    far[1] = DIV * (N_DAYS + 3)
    with pytest.raises(KeyError):
        tgn.recommend(users, far, 5, ITEMS, mv=led, portfolios=rows)
    got = tgn.recommend(users, _dev(far), 5, ITEMS, mv=led, portfolios=rows)
    nv = got[2].cpu().numpy()
    assert nv[1] == 0 and (got[0][1] == -1).all() and (nv[np.arange(len(users)) != 1] > 0).all()


def test_appended_days_are_served_and_a_new_stock_enters():
    g, tgn = _world()
    users, ts, rows = _queries(g, tgn)
    rs = np.random.RandomState(9)
    led = P.PriceLedger.from_prices(np.arange(N_DAYS), g.prices, g.upper_u, DEV, max_days=N_DAYS, key_divisor=DIV)
    mv = P.MVSampler(g.prices, g.upper_u, DEV, day_of=g.day_of)
    new_node = tgn.add_nodes(1)
    assert new_node == N_USERS + N_ITEMS + 1 and new_node - g.upper_u - 1 == N_ITEMS
    items = np.concatenate([ITEMS, [new_node]])
    k = len(items)
    before = _model_state(tgn)

    def reference():
        st = led.state()
        first = int(st["day_keys"][0])
        assert np.array_equal(st["day_keys"], first + np.arange(led.n_days))
        return types.SimpleNamespace(returns=st["returns"], upper_u=g.upper_u, gamma=led.gamma, lambda_mv=led.lambda_mv,
                                     day_of=lambda t: (PR.keys_of(t, DIV) - first).astype(np.int32))

    def offered(mv_, t_arg, **kw):
        out = tgn.recommend(users, t_arg, k, items, mv=mv_, **dict(dict(portfolios=rows), **kw))
        return out, bool((out[0] == new_node).any())

    close = g.prices[-1, :, -1].copy()
    ts_new = ts.copy()
    for day in range(3):
        ref_mv = reference()
        for name, kw in FORMS:
            want, _ = offered(ref_mv, ts_new, **kw)
            for t_arg in (ts_new, _dev(ts_new)):
                got, has_new = offered(led, t_arg, **kw)
                assert all(torch.equal(a, b) for a, b in zip(got, want)), "%s after %d appended days" % (name, day)
                # not quoted yet (day 0: outside the table; day 1: one close, a constant series) - offered after two closes
                assert has_new == (day == 2), "the new stock after %d quotes" % day
        assert not offered(mv, ts, )[1], "never offered with an MVSampler"
        if day == 2:
            break
        # the next trading day: every stock moves, the new stock is quoted (sparse form on odd days, from the device)
        close = close * np.exp(rs.randn(N_ITEMS) * 0.02)
        key = N_DAYS + day
        if day == 0:
            led.append_day(key, np.concatenate([close, [42.0]]))
        else:
            idx = rs.permutation(N_ITEMS + 1).astype(np.int32)
            led.append_day(key, _dev(np.concatenate([close, [43.5]])[idx]), _dev(idx))
        assert led.n_days == N_DAYS and led.head == day + 1 and led.n_stocks == N_ITEMS + 1
        ts_new = ts.copy()
        ts_new[::2] = DIV * key + 1000.0 * np.arange(len(ts_new[::2]) ) % 3000       # some users on the new day, the others on old ones
    tab = led.state()["returns"]
    assert not tab[:-1, N_ITEMS].any() and tab[-1, N_ITEMS, -1] != 0 and not tab[-1, N_ITEMS, :-1].any()
    assert _unchanged(tgn, before), "a query and a tick of the price ledger write no model state"
