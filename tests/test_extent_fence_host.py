"""The extent fences themselves (tests/extent_fence.py), on the CPU: shape, stride and alignment of the view, a fresh fence is
intact, and a change of any single guard element -- before the view, behind it, in the pitch columns; a different NaN included --
is reported at its place."""
import pytest
import torch

from extent_fence import GUARD_ELEMS, GUARD_ROWS, POISON, assert_intact, fence_in, fenced, unwritten

DTYPES = [torch.float32, torch.float16, torch.int32, torch.int64, torch.uint8]
# columns / pitch per dtype: the pitch a multiple of 16 bytes and wider than the view
SHAPE = {torch.float32: (96, 104), torch.float16: (96, 128), torch.int32: (20, 24), torch.int64: (3, 6), torch.uint8: (19, 32)}


def _other(dtype, kind):
    """a value that differs from the poison: for the float types ANOTHER quiet NaN (one payload bit flipped)"""
    p = POISON[kind][dtype]
    if dtype == torch.float32:
        return torch.tensor([p ^ 1], dtype=torch.int32).view(torch.float32)[0]
    if dtype == torch.float16:
        return torch.tensor([p ^ 1], dtype=torch.int16).view(torch.float16)[0]
    return torch.tensor(7, dtype=dtype)


def test_guards_cover_the_largest_row_tile():
    assert GUARD_ROWS >= 256 + 128 and GUARD_ELEMS % 16 == 0 and GUARD_ELEMS >= 256
    for dtype in DTYPES:
        assert POISON["in"][dtype] != POISON["out"][dtype]
    for kind in ("in", "out"):                                # the float poisons are NaNs, quiet ones
        f32 = torch.tensor([POISON[kind][torch.float32]], dtype=torch.int32).view(torch.float32)
        f16 = torch.tensor([POISON[kind][torch.float16]], dtype=torch.int16).view(torch.float16)
        assert bool(torch.isnan(f32).all()) and bool(torch.isnan(f16).all())
        assert POISON[kind][torch.float32] & 0x00400000 and POISON[kind][torch.float16] & 0x0200


@pytest.mark.parametrize("kind", ["out", "in"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_fence_2d(dtype, kind):
    cols, pitch = SHAPE[dtype]
    rows = 5
    v = fenced(rows, cols, dtype, pitch=pitch, kind=kind)
    f = v.fence
    assert tuple(v.shape) == (rows, cols) and v.stride() == (pitch, 1) and v.dtype == dtype
    assert v.data_ptr() % 16 == 0 and f.guard == GUARD_ROWS
    assert v.data_ptr() - f.buf.data_ptr() == GUARD_ROWS * pitch * v.element_size()
    assert f.buf.numel() == (2 * GUARD_ROWS + rows) * pitch
    assert_intact(v)
    assert unwritten(v) == rows * cols
    v.zero_()                                                 # writing the whole view is no change of the guard
    assert_intact(v)
    assert unwritten(v) == 0
    whole = f.buf.view(-1, pitch)
    g = GUARD_ROWS
    # one element each: the rows before, the rows behind, the pitch columns; first and last guard element of the allocation
    for r, c in [(-1, 3), (-g, 0), (rows, 0), (rows + g - 1, pitch - 1), (0, cols), (rows - 1, pitch - 1), (2, cols + 1)]:
        for value in (torch.tensor(1, dtype=dtype), _other(dtype, kind)):
            keep = whole[g + r, c].clone()
            whole[g + r, c] = value
            assert f.changed() == (r, c), (r, c)
            assert f.changed_rows() == [r]
            with pytest.raises(AssertionError, match=rf"\(row {r}, column {c}\)"):
                assert_intact(v)
            whole[g + r, c] = keep
            assert_intact(v)
    # the FIRST changed element is the one named
    whole[g + rows, 1] = 1
    whole[g - 2, 5] = 1
    assert f.changed() == (-2, 5) and f.changed_rows() == [-2, rows]


@pytest.mark.parametrize("kind", ["out", "in"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_fence_1d(dtype, kind):
    n = 37
    v = fenced(n, None, dtype, kind=kind)
    f = v.fence
    assert tuple(v.shape) == (n,) and v.stride() == (1,) and v.dtype == dtype and v.data_ptr() % 16 == 0
    assert f.buf.numel() == 2 * GUARD_ELEMS + n
    assert_intact(v)
    v.zero_()
    assert_intact(v)
    g = GUARD_ELEMS
    for i in (-1, -g, n, n + g - 1):
        for value in (torch.tensor(1, dtype=dtype), _other(dtype, kind)):
            keep = f.buf[g + i].clone()
            f.buf[g + i] = value
            assert f.changed() == (i, 0) and f.changed_rows() == [i]
            with pytest.raises(AssertionError, match=rf"\(row {i}, column 0\)"):
                assert_intact(v)
            f.buf[g + i] = keep
            assert_intact(v)


def test_fence_in_holds_the_values_and_pitches_are_checked():
    x = torch.arange(15, dtype=torch.float32).reshape(3, 5)
    v = fence_in(x, pitch=8)
    assert torch.equal(v, x) and v.fence.kind == "in" and v.stride() == (8, 1)
    assert_intact(v)
    i = fence_in(torch.arange(9, dtype=torch.int64))
    assert torch.equal(i, torch.arange(9)) and i.fence.cols is None
    assert_intact(v, i)
    with pytest.raises(ValueError):
        fenced(3, 5, torch.float32, pitch=6)                  # 24 bytes: the view's rows would not be 16-byte aligned
    with pytest.raises(ValueError):
        fenced(3, 5, torch.float16, pitch=4)                  # narrower than the view
    with pytest.raises(ValueError):
        fenced(3, None, torch.uint8, guard_rows=8)
    # an input guard copied into an output guard is a change of the output fence
    o = fenced(3, 5, torch.float32, pitch=8)
    o.fence.buf.view(-1, 8)[o.fence.guard + 3] = v.fence.buf.view(-1, 8)[v.fence.guard + 3]
    assert o.fence.changed() == (3, 0)
