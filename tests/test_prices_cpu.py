"""CPU side of the price ledger: the numpy reference against a plain Python loop over days, the day-key rule
against ``str(ts)[:8]``, every host-side refusal of ``PriceLedger`` (raised before any device work - a refused call leaves the
ledger bit for bit), ``from_prices`` against ``log_returns``, the capacity scheme on CPU tensors and the ledger branch of
``recommend.validate``.  No kernel runs here."""
import os
import re

import numpy as np
import pytest
import torch

import prices_ref as PR
from conftest import REPO

SYMBOLS = ("pfo_returns_append_day", "pfo_returns_scatter_closes", "pfo_returns_scatter_scratch_bytes", "pfo_day_lookup")
UPPER_U = 50


# ---------------------------------------------------------------------------------------------- 1. the reference's own rules
def _loop_table(days, n_ret):
    """Plain Python: per stock the list of its daily returns; the window of a day is the newest n_ret of them behind zeros."""
    n_stocks = max(len(c) for _, c in days)
    hist, last, out = [[] for _ in range(n_stocks)], [None] * n_stocks, []
    for d, (_, closes) in enumerate(days):
        for s in range(n_stocks):
            c = closes[s] if s < len(closes) else float("nan")
            r = 0.0
            if c == c:
                if last[s] is not None:
                    r = float(np.log(np.float64(c) / np.float64(last[s])))
                last[s] = c
            hist[s].append(r if d > 0 else 0.0)
        out.append([([0.0] * n_ret + h)[-n_ret:] for h in hist])
    return np.array(out), np.array([np.nan if v is None else v for v in last])


@pytest.mark.parametrize("n_ret", [2, 5])
def test_reference_is_the_plain_loop(n_ret):
    rs = np.random.RandomState(n_ret)
    days = []
    for d in range(9):
        n = 4 if d < 3 else 6                                     # two stocks join on day 3
        c = 50.0 * np.exp(rs.randn(n) * 0.1)
        c[rs.rand(n) < 0.3] = np.nan                              # not quoted today
        if d >= 3:
            c[5] = np.nan if d < 6 else c[5]                      # stock 5: listed on day 3, first quoted on day 6
        days.append((20240100 + d, c))
    days[4][1][0] = days[3][1][0] = 77.0                          # a quotient of exactly 1.0 (when both are quoted)
    ref = PR.RefLedger(n_ret)
    for key, c in days:
        ref.append_day(key, c)
    want, last = _loop_table(days, n_ret)
    assert ref.n_days == 9 and ref.day_cap == 16 and ref.head == 0
    assert PR.same_bits(ref.table, want) and PR.same_bits(ref.last_close, last)
    assert not ref.table[0].any(), "the first day of an empty ledger is all zeros"
    assert not ref.table[:6, 5].any() and not ref.table[6, 5].any(), "a stock first quoted mid-history starts at +0"
    assert not np.signbit(ref.table).any() or (ref.table[np.signbit(ref.table)] != 0).all(), "no -0 anywhere"
    # the sparse form is the dense one
    sp = PR.RefLedger(n_ret)
    for key, c in days:
        idx = np.flatnonzero(~np.isnan(c))[::-1]
        sp._grow_stocks(len(c))
        sp.append_day(key, c[idx], idx)
    assert PR.same_bits(sp.table, ref.table) and PR.same_bits(sp.last_close, ref.last_close)


def test_reference_ring_expiry_and_skip_rules():
    ref = PR.RefLedger(3, max_days=2)
    full = PR.RefLedger(3)
    rs = np.random.RandomState(0)
    for d in range(5):
        c = 10.0 + rs.rand(3)
        ref.append_day(d, c)
        full.append_day(d, c)
    assert ref.day_cap == 2 and ref.n_days == 2 and ref.keys.tolist() == [3, 4]
    assert PR.same_bits(ref.table, full.table[3:]), "the shift reaches through days that have left the ring"
    one = PR.RefLedger(3, max_days=1)
    for d in range(5):
        one.append_day(d, full.last_close if d == 4 else 10.0 + np.arange(3.0) + d)
    assert one.day_cap == 2 and one.n_days == 1 and one.keys.tolist() == [4]
    assert full.expire_days(2) == 2 and full.keys.tolist() == [2, 3, 4] and full.head == 2
    assert full.expire_days(0) == 0 and full.expire_days(3) == 1 and full.expire_days(99) == 2 and full.n_days == 0
    # unchecked (device) inputs: skipped positions, the last valid one wins, no growth
    r = PR.RefLedger(2)
    r.append_day(1, [5.0, 5.0, 5.0])
    q = r.append_day(2, [6.0, 7.0, -1.0, 8.0, np.inf, 0.0, 9.0, np.nan], [0, 0, 0, 3, 1, 1, -1, 2], grow=False)
    assert r.n_stocks == 3 and r.last_close.tolist() == [7.0, 5.0, 5.0] and q[0] == 7.0 / 5.0 and np.isnan(q[1:]).all()
    assert r.lookup([2.5e6, 1e6, 3e6, 0.0]).tolist() == [1, 0, -1, -1]


# ---------------------------------------------------------------------------------------------- 2. the day-key rule
def test_day_key_is_the_first_eight_digits():
    rs = np.random.RandomState(3)
    n = 200000
    ymd = rs.randint(19000101, 99991231, size=n).astype(np.int64)
    hms = rs.randint(0, 1000000, size=n).astype(np.int64)
    hms[:30000] = 0
    hms[30000:60000] = 235959
    hms[60000:90000] = 999999
    ymd[:3], ymd[-3:] = [10000000, 99999999, 10000000], [99999999, 20240229, 20231231]
    ts = ymd * 1000000 + hms
    want = np.array([int(str(t)[:8]) for t in ts.tolist()], np.int64)
    assert np.array_equal(want, ymd)
    assert np.array_equal(PR.keys_of(ts), want), "integer timestamps"
    assert np.array_equal(PR.keys_of(ts.astype(np.float64)), want), "the same as fp64, what the device sees"
    import pfotgnrec_amd as P
    from pfotgnrec_amd.mv_sampler import day_indices
    led = P.PriceLedger(4, UPPER_U, "cpu")
    assert np.array_equal(led.keys_of(ts), want) and np.array_equal(led.keys_of(ts.astype(np.float64)), want)
    days = np.unique(ymd)
    led.load_state(dict(day_keys=days, returns=np.zeros((len(days), 1, 4)), last_close=np.ones(1)))
    assert np.array_equal(led.day_of(ts[:5000]), day_indices(ts[:5000], days.tolist()))


# ---------------------------------------------------------------------------------------------- 3. symbols
def test_symbols_in_header_library_and_prototypes():
    from pfotgnrec_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "pfotgn.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name) and name in _lib.PROTOTYPES, name
    assert lib.pfo_abi_version() == 6 and "prices.hip" in build.SOURCES
    import pfotgnrec_amd as P
    assert all(hasattr(P, n) for n in ("PriceLedger", "returns_append_day", "returns_scatter_closes", "day_lookup"))
    assert lib.pfo_returns_scatter_scratch_bytes(300) == 1200 and lib.pfo_returns_scatter_scratch_bytes(-1) == -1


def test_limits_are_refused_before_anything_is_dereferenced():
    from pfotgnrec_amd import _lib
    ok = dict(day_cap=4, stock_cap=8, n_ret=5, prev=0, new=1, n_stocks=8, n_closes=8)

    def append(**kw):
        a = dict(ok, **kw)
        _lib.call("pfo_returns_append_day", None, a["day_cap"], a["stock_cap"], a["n_ret"], a["prev"], a["new"], a["n_stocks"], None,
                  a["n_closes"], None, None, None, 7, None, None)
    for kw, msg in ((dict(day_cap=1), "day_cap"), (dict(n_ret=1), "n_ret"), (dict(n_ret=129), "n_ret"), (dict(stock_cap=0), "stock_cap"),
                    (dict(n_stocks=9), "n_stocks"), (dict(new=4), "new_slot"), (dict(new=-1), "new_slot"), (dict(prev=-2), "prev_slot"),
                    (dict(prev=1), "shifted from"), (dict(n_closes=-1), "n_closes"), ({}, "null pointer")):
        with pytest.raises(_lib.PfoError, match=msg):
            append(**kw)

    def lookup(U=1, cap=4, head=0, n=2, div=1e6):
        _lib.call("pfo_day_lookup", None, U, None, cap, head, n, div, None, None)
    for kw, msg in ((dict(U=-1), "U must"), (dict(cap=0), "day_cap"), (dict(n=5), "n_days"), (dict(head=4), "head"), (dict(div=0.0), "key_divisor"),
                    (dict(div=float("nan")), "key_divisor"), ({}, "null pointer")):
        with pytest.raises(_lib.PfoError, match=msg):
            lookup(**kw)
    lookup(U=0)
    with pytest.raises(_lib.PfoError, match="m must"):
        _lib.call("pfo_returns_scatter_closes", None, None, -1, 5, None, 20, None)
    with pytest.raises(_lib.PfoError, match="null pointer"):
        _lib.call("pfo_returns_scatter_closes", None, None, 1, 5, None, 20, None)
    _lib.call("pfo_returns_scatter_closes", None, None, 3, 0, None, 0, None)


# ---------------------------------------------------------------------------------------------- 4. the Python surface on the host
def _seeded(max_days=None, days=5, stocks=6, P_=6):
    import pfotgnrec_amd as P
    rs = np.random.RandomState(days)
    prices = 100.0 * np.exp(np.cumsum(rs.randn(days, stocks, P_) * 0.02, axis=2))
    keys = 20240101 + np.arange(days)
    return P.PriceLedger.from_prices(keys, prices, UPPER_U, "cpu", max_days=max_days), keys, prices


def _snapshot(led):
    return (led.head, led.n_days, led.n_stocks, led.day_cap, led.stock_cap, list(led.keys), led.returns.data_ptr(),
            led.returns.numpy().tobytes(), led.day_keys.numpy().tobytes(), led.last_close.numpy().tobytes())


def test_from_prices_is_log_returns_bit_for_bit():
    from pfotgnrec_amd.mv_sampler import log_returns
    led, keys, prices = _seeded()
    st = led.state()
    assert PR.same_bits(st["returns"], log_returns(prices)) and PR.same_bits(st["day_keys"], keys.astype(np.int64))
    assert PR.same_bits(st["last_close"], prices[-1, :, -1])
    assert (led.n_ret, led.n_days, led.n_stocks, led.stock_cap, led.day_cap, led.head) == (5, 5, 6, 6, 5, 0)
    assert tuple(led.returns.shape) == (5, 6, 5) and led.returns.dtype == torch.float64
    assert led.upper_u == UPPER_U and led.gamma == 2.0 and led.lambda_mv == 0.5 and callable(led.day_of)
    import pfotgnrec_amd as P
    for bad in (dict(day_keys=keys[:4]), dict(day_keys=keys[::-1]), dict(prices=prices[:, :, :2]), dict(prices=prices[0]),
                dict(day_keys=keys + 0.5), dict(max_days=4)):
        kw = dict(dict(day_keys=keys, prices=prices, upper_u=UPPER_U, device="cpu"), **bad)
        with pytest.raises(ValueError):
            P.PriceLedger.from_prices(**kw)
    for bad in (dict(n_ret=1), dict(n_ret=129), dict(max_days=0), dict(key_divisor=0.0), dict(key_divisor=float("inf")), dict(n_ret=2.5)):
        with pytest.raises(ValueError):
            P.PriceLedger(**dict(dict(n_ret=5, upper_u=UPPER_U, device="cpu"), **bad))


BAD_DAYS = ["key_not_above", "key_equal", "key_float", "close_zero", "close_negative", "close_inf", "dense_short", "dense_2d",
            "sparse_nan", "sparse_negative_index", "sparse_index_beyond_int32", "sparse_repeated", "sparse_length", "sparse_float_index",
            "sparse_mixed_residence", "closes_strings", "device_dtype", "device_sparse_dtype", "device_sparse_shape", "device_dense_short"]


@pytest.mark.parametrize("case", BAD_DAYS)
def test_rejected_append_day_leaves_everything(case):
    led, keys, _ = _seeded()
    key, closes, stocks = int(keys[-1]) + 1, np.full(6, 10.0), None
    if case == "key_not_above":
        key = int(keys[0])
    elif case == "key_equal":
        key = int(keys[-1])
    elif case == "key_float":
        key = 20240110.0
    elif case == "close_zero":
        closes[2] = 0.0
    elif case == "close_negative":
        closes[2] = -3.0
    elif case == "close_inf":
        closes[2] = np.inf
    elif case == "dense_short":
        closes = closes[:5]
    elif case == "dense_2d":
        closes = closes.reshape(2, 3)
    elif case == "closes_strings":
        closes = np.array(["1"] * 6)
    elif case == "device_dtype":
        closes = torch.full((6,), 10.0, dtype=torch.float32)
    elif case == "device_dense_short":
        closes = torch.full((5,), 10.0, dtype=torch.float64)
    elif case == "device_sparse_dtype":
        closes, stocks = torch.full((2,), 10.0, dtype=torch.float64), torch.zeros(2, dtype=torch.int64)
    elif case == "device_sparse_shape":
        closes, stocks = torch.full((2,), 10.0, dtype=torch.float64), torch.zeros(3, dtype=torch.int32)
    else:
        closes, stocks = np.array([10.0, 11.0, 12.0]), np.array([1, 4, 7])
        if case == "sparse_nan":
            closes[1] = np.nan
        elif case == "sparse_negative_index":
            stocks[0] = -1
        elif case == "sparse_index_beyond_int32":
            stocks[2] = 2 ** 31 - 1
        elif case == "sparse_repeated":
            stocks[2] = 1
        elif case == "sparse_length":
            stocks = stocks[:2]
        elif case == "sparse_float_index":
            stocks = stocks.astype(np.float64)
        elif case == "sparse_mixed_residence":
            stocks = torch.from_numpy(stocks.astype(np.int32))
    before = _snapshot(led)
    with pytest.raises(ValueError):
        led.append_day(key, closes, stocks)
    assert _snapshot(led) == before


def test_valid_append_reaches_the_device_check_and_changes_nothing_on_a_host_ledger():
    """There is no CPU implementation: valid arguments pass every check and are refused where the device is asked for, before
    the first table grows."""
    from pfotgnrec_amd import _lib
    led, keys, _ = _seeded()
    before = _snapshot(led)
    dense = np.full(9, 10.0)                                      # three new stocks: the table would have to grow
    dense[3] = np.nan
    for closes, stocks in ((dense, None), (np.array([3.0, 4.0]), np.array([8, 0])), (torch.full((6,), 10.0, dtype=torch.float64), None),
                           (torch.full((2,), 10.0, dtype=torch.float64), torch.zeros(2, dtype=torch.int32))):
        with pytest.raises(_lib.PfoError):
            led.append_day(int(keys[-1]) + 1, closes, stocks)
    with pytest.raises(_lib.PfoError):
        led.lookup(torch.zeros(3, dtype=torch.float64))
    assert _snapshot(led) == before


def test_day_of_expire_reserve_and_state_on_the_host():
    led, keys, prices = _seeded()
    ts = np.array([20240103120000, 20240101000000, 20240105235959], np.float64)
    assert led.day_of(ts).tolist() == [2, 0, 4] and led.day_of(ts).dtype == np.int32
    for missing in (20231231235959.0, 20240106000000.0, float("nan")):
        with pytest.raises(KeyError):
            led.day_of(np.array([20240102000000.0, missing]))
    st = led.state()
    # reserve: live rows bit for bit, capacity never shrinks, less than live is refused
    for bad in (dict(n_days=4), dict(n_stocks=5), dict(n_days=2.5), dict(n_stocks=2 ** 31)):
        before = _snapshot(led)
        with pytest.raises(ValueError):
            led.reserve(**bad)
        assert _snapshot(led) == before
    ptr = led.returns.data_ptr()
    led.reserve(n_days=5, n_stocks=6)
    led.reserve()
    assert led.returns.data_ptr() == ptr, "nothing to do: nothing moves"
    led.reserve(n_days=9)
    led.reserve(n_stocks=11)
    led.reserve(n_days=6, n_stocks=7)                             # below capacity: kept
    assert (led.day_cap, led.stock_cap, led.n_days, led.n_stocks) == (9, 11, 5, 6)
    assert all(PR.same_bits(st[k], led.state()[k]) for k in st)
    full = led.returns.numpy()
    assert not full[5:].any() and not full[:, 6:].any(), "rows behind the live counts are zeros"
    assert np.isnan(led._last_close.numpy()[6:]).all() and led.last_close.shape[0] == 6
    # expiry moves head alone
    before_bits = led.returns.numpy().tobytes()
    assert led.expire_days(int(keys[0])) == 0 and led.expire_days(int(keys[2])) == 2
    assert (led.head, led.n_days, led.keys) == (2, 3, keys[2:].tolist()) and led.returns.numpy().tobytes() == before_bits
    assert led.day_of(ts[:1]).tolist() == [0]
    with pytest.raises(KeyError):
        led.day_of(ts[1:2])                                       # just expired
    assert led.slots_of(np.array([0, 2, 3, -1])).tolist() == [2, 4, -1, -1]
    assert led.slots_of(torch.tensor([0, 2, 3, -1])).tolist() == [2, 4, -1, -1]
    assert PR.same_bits(led.state()["returns"], st["returns"][2:])
    # a re-layout of a ring whose head is not 0
    led.reserve(n_days=12)
    assert led.head == 0 and PR.same_bits(led.state()["returns"], st["returns"][2:]) and led.keys == keys[2:].tolist()
    assert led.expire_days(10 ** 9) == 3 and led.n_days == 0 and led.state()["returns"].shape == (0, 6, 5)
    # state -> load_state -> state, into a ledger of another shape
    import pfotgnrec_amd as P
    other = P.PriceLedger(5, UPPER_U, "cpu", max_days=7)
    other.load_state(st)
    assert all(PR.same_bits(st[k], other.state()[k]) for k in st) and other.day_cap == 7
    for bad in (dict(day_keys=st["day_keys"][:3]), dict(returns=st["returns"][:, :, :4]), dict(last_close=st["last_close"][:2]),
                dict(returns=st["returns"].astype(np.float32)), dict(day_keys=st["day_keys"][::-1].copy())):
        before = _snapshot(other)
        with pytest.raises(ValueError):
            other.load_state(dict(st, **bad))
        assert _snapshot(other) == before
    with pytest.raises(ValueError):
        other.load_state({"day_keys": st["day_keys"]})


# ---------------------------------------------------------------------------------------------- 5. recommend.validate
def test_ledger_branch_of_recommend_validate():
    import pfotgnrec_amd as P
    from pfotgnrec_amd import recommend as R
    from pfotgnrec_amd.holdings import Holdings
    led, keys, _ = _seeded()
    led.expire_days(int(keys[1]))                                 # 4 live days, head 1
    users, items = np.arange(1, 4), np.arange(51, 57)
    ports = [[0], [1, 2], []]
    v = lambda **kw: R.validate(61, 4, users, kw.pop("ts", 5.0), 3, items, kw.pop("exclude", None), None, None, led, kw.pop("portfolios", ports),
                                kw.pop("day_idx", None), kw.pop("holdings", None), kw.pop("basket", False))
    # explicit ordinals count the LIVE days
    assert v(day_idx=3).mv.day_idx.tolist() == [3, 3, 3] and v(day_idx=[0, 3, 1]).mv.day_idx.tolist() == [0, 3, 1]
    for bad in (4, -1, [0, 1, 4], [0, 1], 1.0):
        with pytest.raises(ValueError):
            v(day_idx=bad)
    q = v(day_idx=torch.tensor([0, 9, 1]))
    assert torch.is_tensor(q.mv.day_idx), "a device day_idx is not read back: an ordinal outside the live days becomes slot -1"
    # host timestamps go through day_of (ordinals; KeyError for a day that is not held), a scalar is broadcast
    ts = np.array([20240104101500.0, 20240102000000.0, 20240105235959.0])
    assert v(ts=ts).mv.day_idx.tolist() == [2, 0, 3] and v(ts=ts[0]).mv.day_idx.tolist() == [2, 2, 2]
    with pytest.raises(KeyError):
        v(ts=np.array([20240104101500.0, 20240101000000.0, 20240105235959.0]))
    # device timestamps: no day index on the host at all - the lookup is the device's
    q = v(ts=torch.from_numpy(ts))
    assert q.mv.src is led and q.mv.day_idx is None
    assert v(ts=torch.tensor(20240104101500.0, dtype=torch.float64)).mv.day_idx is None
    # ... which any other mv still refuses
    class MV:
        returns, upper_u, gamma, lambda_mv = np.zeros((2, 10, 5)), UPPER_U, 1.0, 0.5
        day_of = staticmethod(lambda t: np.zeros(len(t), np.int64))
    with pytest.raises(ValueError, match="timestamps on the host"):
        R.validate(61, 4, users, torch.from_numpy(ts), 3, items, None, None, None, MV, ports, None)
    assert R.validate(61, 4, users, ts, 3, items, None, None, None, MV, ports, None).mv.day_idx.tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match=r"outside \[0, 2\)"):
        R.validate(61, 4, users, ts, 3, items, None, None, None, MV, ports, 2)
    # "held" with a ledger: needs the holdings ledger, the same upper_u - and "held" without mv is still refused
    hold = Holdings(61, 61, 4, UPPER_U, "cpu")
    q = v(portfolios="held", exclude="held", holdings=hold, basket=True, day_idx=1)
    assert q.held == (True, True) and q.basket and q.mv.port_idx is None
    with pytest.raises(ValueError, match="track_holdings"):
        v(portfolios="held")
    with pytest.raises(ValueError, match="upper_u"):
        v(portfolios="held", holdings=Holdings(61, 61, 4, UPPER_U + 1, "cpu"))
    with pytest.raises(ValueError, match="need mv"):
        R.validate(61, 4, users, 5.0, 3, items, None, None, None, None, "held", None, hold)
    with pytest.raises(ValueError, match="needs portfolios"):
        v(portfolios=None)
