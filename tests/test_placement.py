"""The placement helper itself (tests/placement.py), on host tensors: the
views lie where they claim to, and check_guards catches a write on either side
of a view, also one that touches a single field of a tuple."""
import types

import numpy as np
import pytest

import placement
from placement import GUARD, SENTINEL, arena, arena_column, check_guards

DTYPES = {8: np.dtype([("payload", "<i4"), ("key", "<i4")]),
          16: np.dtype([("payload", "<i8"), ("key", "<i8")])}


def host_lib(width):
    return types.SimpleNamespace(width=width, dtype=DTYPES[width])


def test_sentinel_is_the_matrix_one():
    import test_gpu_layout_matrix as m
    assert placement.SENTINEL == m.SENTINEL and placement.GUARD == m.CANARY


@pytest.mark.parametrize("n", [0, 1, 77])
@pytest.mark.parametrize("off", [0, 1, 3])
def test_view_offsets(width, off, n):
    lib = host_lib(width)
    t = np.zeros(n, DTYPES[width])
    t["key"] = np.arange(n) + 1
    t["payload"] = -np.arange(n)
    buf, view = arena(lib, n, off, fill=t, device="cpu")
    assert buf.shape == (GUARD + off + n + GUARD, 2) and view.shape == (n, 2)
    assert buf.data_ptr() % 256 == 0
    assert view.data_ptr() - buf.data_ptr() == (GUARD + off) * width
    assert view.data_ptr() % 64 == (off * width) % 64
    if width == 8 and off % 2:
        assert view.data_ptr() % 16 == 8
    h = buf.numpy()
    assert np.array_equal(h[GUARD + off:GUARD + off + n, 1], t["key"])
    assert np.array_equal(h[GUARD + off:GUARD + off + n, 0], t["payload"])
    assert (h[:GUARD + off] == SENTINEL).all() and (h[GUARD + off + n:] == SENTINEL).all()
    check_guards(buf, view, "untouched")
    cbuf, col = arena_column(lib, n, off, device="cpu")
    assert col.data_ptr() - cbuf.data_ptr() == (GUARD + off) * (width // 2)
    check_guards(cbuf, col, "untouched column")


@pytest.mark.parametrize("n", [0, 5])
@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("where", ["before", "behind", "payload_before", "key_behind",
                                   "first_guard", "last_guard"])
def test_check_guards_catches_planted_writes(width, off, n, where):
    lib = host_lib(width)
    buf, view = arena(lib, n, off, device="cpu")
    view.fill_(7)
    check_guards(buf, view, "clean")
    row, cols = {"before": (GUARD + off - 1, (0, 1)), "behind": (GUARD + off + n, (0, 1)),
                 "payload_before": (GUARD + off - 1, (0,)), "key_behind": (GUARD + off + n, (1,)),
                 "first_guard": (0, (0, 1)), "last_guard": (buf.shape[0] - 1, (0, 1))}[where]
    for c in cols:
        buf[row, c] = 7
    with pytest.raises(AssertionError, match="planted"):
        check_guards(buf, view, "planted")


@pytest.mark.parametrize("where", ["before", "behind"])
def test_check_guards_on_columns(width, where):
    lib = host_lib(width)
    buf, col = arena_column(lib, 9, 3, device="cpu")
    col.fill_(0)
    check_guards(buf, col, "clean")
    buf[GUARD + 3 - 1 if where == "before" else GUARD + 3 + 9] = 0
    with pytest.raises(AssertionError, match="planted"):
        check_guards(buf, col, "planted")
