"""``tables.RowStore`` on host tensors: the one rule of a table that grows - how storage with spare capacity is allocated, what
the rows behind the live count hold, how live rows cross a reallocation, how the views are re-made - at the smallest shapes at
which each part can go wrong: three tensors of three rows with a matrix, a byte and an fp64 column with a non-zero fill."""
import numpy as np
import pytest
import torch

from pfotgnrec_amd.tables import RowStore, _grown

FILLS = (0, 0, float("-inf"))


def _tensors():
    rs = np.random.RandomState(3)
    return [torch.from_numpy(rs.randn(3, 2).astype(np.float32)), torch.tensor([1, 0, 255], dtype=torch.uint8),
            torch.from_numpy(rs.randn(3))]


def _bytes(tensors):
    return [t.numpy().tobytes() for t in tensors]


def _tail_is_fill(store, lo):
    a, b, c = (t[lo:] for t in store.storage)
    return not a.any() and not b.any() and bool(torch.isneginf(c).all())


def _same_layout(views, like, rows):
    return all(v.is_contiguous() and v.dtype == t.dtype and tuple(v.shape) == (rows,) + tuple(t.shape[1:]) for v, t in zip(views, like))


def test_adopting_full_tensors_copies_nothing():
    tensors = _tensors()
    store = RowStore(tensors, FILLS)
    assert (store.capacity, store.rows) == (3, 3)
    assert [v.data_ptr() for v in store.views()] == [t.data_ptr() for t in tensors]
    assert _same_layout(store.views(), tensors, 3) and _bytes(store.views()) == _bytes(tensors)


def test_reserve_allocates_exactly_copies_live_rows_and_fills_the_tail():
    tensors = _tensors()
    store, before = RowStore(tensors, FILLS), _bytes(tensors)
    assert store.reserve(5) is True
    assert (store.capacity, store.rows) == (5, 3) and all(t.shape[0] == 5 for t in store.storage)
    views = store.views()
    assert _bytes(views) == before, "live rows are equal as bytes"
    assert _tail_is_fill(store, 3), "rows 3 and 4 hold the fills, -inf in the f64 tensor"
    assert _same_layout(views, tensors, 3)
    assert [v.data_ptr() for v in views] == [t.data_ptr() for t in store.storage]
    assert all(v.data_ptr() != t.data_ptr() for v, t in zip(views, tensors)), "the storage moved"
    # the same request again, or a smaller one, moves nothing: capacity never shrinks
    ptrs = [t.data_ptr() for t in store.storage]
    assert store.reserve(5) is False and store.reserve(4) is False and store.reserve(0) is False
    assert store.capacity == 5 and [t.data_ptr() for t in store.storage] == ptrs


def test_the_live_count_only_grows_within_the_capacity():
    store = RowStore(_tensors(), FILLS)
    store.reserve(5)
    ptrs, before = [t.data_ptr() for t in store.storage], _bytes(store.storage)
    store.set_rows(5)
    assert store.rows == 5 and [v.shape[0] for v in store.views()] == [5, 5, 5]
    assert [v.data_ptr() for v in store.views()] == ptrs and _bytes(store.storage) == before, "re-sliced, nothing moved"
    assert _tail_is_fill(store, 3), "the rows that came alive start from the fills"
    with pytest.raises(ValueError, match="capacity"):          # this store's contract: beyond the capacity is refused
        store.set_rows(6)
    for fewer in (4, 0):
        with pytest.raises(ValueError, match="do not shrink"):
            store.set_rows(fewer)
    with pytest.raises(ValueError, match="do not shrink"):
        store.resize(4)
    assert (store.rows, store.capacity) == (5, 5) and [t.data_ptr() for t in store.storage] == ptrs
    store.set_rows(5)                                           # (the present count is no shrink)


def test_trim_is_the_one_way_down():
    store = RowStore(_tensors(), FILLS)
    store.reserve(5)
    store.set_rows(5)
    ptrs = [t.data_ptr() for t in store.storage]
    store.trim(2)
    assert (store.rows, store.capacity) == (2, 5) and [v.shape[0] for v in store.views()] == [2, 2, 2]
    assert [v.data_ptr() for v in store.views()] == ptrs
    with pytest.raises(ValueError):
        store.trim(3)                                           # (trim never adds rows)
    with pytest.raises(ValueError):
        store.trim(-1)
    store.set_rows(4)                                           # growth continues from the trimmed count
    assert store.rows == 4


def test_resize_grows_just_enough_or_to_the_capacity_asked_for():
    store = RowStore(_tensors(), FILLS)
    assert store.resize(3) is False and store.capacity == 3
    assert store.resize(4) is True and (store.rows, store.capacity) == (4, 4), "None: just enough"
    assert store.resize(4, 9) is True and (store.rows, store.capacity) == (4, 9)
    assert store.resize(6, 2) is False and (store.rows, store.capacity) == (6, 9), "a smaller capacity is what is there"
    assert _tail_is_fill(store, 3)


def test_allocate_starts_from_the_fills():
    specs = [((2,), torch.float32, 0), ((), torch.uint8, 0), ((), torch.float64, float("-inf"))]
    store = RowStore.allocate(specs, 5, 3, "cpu")
    assert (store.capacity, store.rows) == (5, 3) and _tail_is_fill(store, 0)
    assert [tuple(v.shape) for v in store.views()] == [(3, 2), (3,), (3,)]
    assert [v.dtype for v in store.views()] == [torch.float32, torch.uint8, torch.float64]
    store.reserve(7)
    assert store.capacity == 7 and _tail_is_fill(store, 0), "a grown store keeps the fills it was allocated with"
    assert RowStore.allocate(specs, 2, 3, "cpu").capacity == 3, "never less than the live rows"


def test_move_applies_one_function_per_tensor():
    tensors = _tensors()
    store = RowStore(tensors, FILLS)
    store.reserve(5)
    store.set_rows(4)
    cast = lambda t: t.double()
    keep = lambda t: t.to("cpu")
    store.move(cast, keep, keep)
    assert [t.dtype for t in store.storage] == [torch.float64, torch.uint8, torch.float64]
    assert (store.capacity, store.rows) == (5, 4) and all(t.shape[0] == 5 and t.is_contiguous() for t in store.storage)
    assert torch.equal(store.views()[0][:3], tensors[0].double()) and _bytes(v[:3] for v in store.views()[1:]) == _bytes(tensors[1:])
    assert _tail_is_fill(store, 3)
    store.move(keep)                                            # one function for all
    assert [t.dtype for t in store.storage] == [torch.float64, torch.uint8, torch.float64] and (store.capacity, store.rows) == (5, 4)
    with pytest.raises(ValueError):
        store.move(keep, keep)


def test_growth_policy():
    assert _grown(100, 101) == 166 and _grown(0, 1) == 16
    assert _grown(100, 1000) == 1000, "a need above the geometric step wins"
    store = RowStore([torch.zeros(100)])
    assert store.capacity_for(100) == 100 and store.capacity_for(7) == 100, "what is there, while it holds the rows"
    assert store.capacity_for(101) == 166 and store.capacity_for(1000) == 1000
