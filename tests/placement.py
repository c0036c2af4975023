"""Where a test's device buffers lie: a helper of test_placement.py,
test_gpu_layout_matrix.py and test_gpu_placement.py.

arena() gives a view `off` tuples (or elements) into one allocation, with
GUARD sentinel tuples in front of the view and behind it.  An odd `off` puts
an 8-byte tuple at an address that is 8 mod 16: the side of the library's
`((uintptr_t)p & 15) == 0` dispatch tests that fresh allocations never reach.
An over-read or over-write of a few elements stays inside the allocation and
shows as a failed comparison in check_guards().
"""
import numpy as np

GUARD = 64
SENTINEL = 0x5A5A5A5A   # test_gpu_layout_matrix.SENTINEL


def _torch_dtype(lib):
    import torch
    return torch.int32 if lib.width == 8 else torch.int64


def _alloc(rows, per, dtype, device):
    """`rows` rows of sentinels starting at a 256-byte boundary (the device
    allocator's own alignment; the host's is 64 bytes, so skip up to it)."""
    import torch
    esize = torch.empty(0, dtype=dtype).element_size() * per
    spare = 256 // esize
    raw = torch.full((rows + spare, 2) if per == 2 else (rows + spare,), SENTINEL, dtype=dtype,
                     device=device)
    skip = (-raw.data_ptr() % 256) // esize
    return raw[skip:skip + rows]


class _EmptyView:
    """A view of no rows that still knows where it lies: torch gives every
    empty tensor the null pointer.  Everything but data_ptr() is the empty
    tensor's."""

    def __init__(self, t, ptr):
        self._t, self._ptr = t, ptr

    def data_ptr(self):
        return self._ptr

    def __getattr__(self, name):
        return getattr(self._t, name)


def _place(lib, buf, n, off, fill, per):
    """The view of n rows at GUARD + off of `buf`, checked and filled."""
    import torch
    view = buf[GUARD + off:GUARD + off + n]
    esize = buf.element_size() * per
    if n == 0:
        view = _EmptyView(view, buf.data_ptr() + (GUARD + off) * esize)
    assert buf.data_ptr() % 256 == 0, "the allocation itself is aligned"
    assert view.data_ptr() == buf.data_ptr() + (GUARD + off) * esize
    if per == 1:
        pass   # an element column: aligned to its element, nothing to prove
    elif lib.width == 8 and off % 2:
        assert view.data_ptr() % 16 == 8, "an odd offset of 8-byte tuples is misaligned"
    elif lib.width == 16:
        assert view.data_ptr() % 16 == 0
    if fill is not None and n:
        if isinstance(fill, np.ndarray):
            if per == 2:
                fill = np.ascontiguousarray(fill, dtype=lib.dtype).view(
                    np.int32 if lib.width == 8 else np.int64).reshape(-1, 2)
            src = torch.from_numpy(np.array(fill))
        else:
            src = fill
        assert src.shape[0] == n
        view.copy_(src)
    return buf, view


def arena(lib, n, off, fill=None, device="cuda"):
    """(buffer, view): one tensor of GUARD + off + n + GUARD tuples holding
    SENTINEL in both fields, and its rows [GUARD + off, GUARD + off + n), a
    valid pointer also for n == 0.  fill: a structured numpy array or a
    tensor of n tuples copied into the view."""
    buf = _alloc(GUARD + off + n + GUARD, 2, _torch_dtype(lib), device)
    return _place(lib, buf, n, off, fill, 2)


def arena_column(lib, n, off, fill=None, device="cuda", dtype=None):
    """arena() for an element column (value_t / intkey_t outputs, int64
    words): `off` counts elements.  lib may be None where dtype is given."""
    buf = _alloc(GUARD + off + n + GUARD, 1, dtype or _torch_dtype(lib), device)
    return _place(lib, buf, n, off, fill, 1)


def check_guards(buf, view, what):
    """Every tuple (element) of `buf` outside `view` still holds the sentinel,
    in both fields, before and behind the view."""
    per = buf.shape[1] if buf.dim() == 2 else 1
    first = (view.data_ptr() - buf.data_ptr()) // (buf.element_size() * per)
    n = view.shape[0]
    assert first >= GUARD and buf.shape[0] - (first + n) == GUARD, what
    h = buf.cpu().numpy()
    front, back = h[:first], h[first + n:]
    assert (front == SENTINEL).all(), \
        f"{what}: wrote in front of the view at {np.argwhere(front != SENTINEL)[-1].tolist()}"
    assert (back == SENTINEL).all(), \
        f"{what}: wrote behind the {n} elements of the view at " \
        f"+{np.argwhere(back != SENTINEL)[0].tolist()}"
