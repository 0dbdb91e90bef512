"""Extent fences for kernel tests: a tensor view with poisoned guard memory all around it, inside ONE allocation of the test's own.

    y = fenced(nv, d, torch.float32, pitch=d + 8, device="cuda")     # an output: rows x cols, row stride `pitch`
    x = fence_in(x_plain, pitch=d + 8)                               # an input: the same values inside poisoned guards
    kernel(x, x.stride(0), ..., y, y.stride(0))
    assert_intact(y), assert_intact(x)                               # no store outside the extent (and none into an input's guards)

Layout of the 2-D form: [G guard rows][rows x pitch][G guard rows], and the columns cols .. pitch - 1 of every row of the view are
guard as well.  The 1-D form (cols=None) is [G' guard elements][rows elements][G' guard elements].  A kernel that stores a tile too
far, or into the pitch columns, lands in the guard -- inside the allocation, so nothing faults -- and assert_intact names the first
changed element.  A kernel that READS a guard gets the poison: NaN in the float types, so a stray operand shows in the values, which
a test compares bit for bit with the same call on plain tensors.

Arena and run (below) carry a whole case: run(case) calls case(arena) twice -- on plain, contiguous, exactly sized tensors and on
fenced ones -- and asks that the fences are intact and that the two runs' outputs are the same bits.

Poison is a bit pattern per dtype, compared as INTEGERS: overwriting a poison NaN with any other NaN is a change.  Input and output
fences carry different payloads, so a kernel that copies a guard row of its input into a guard row of its output is caught too.
"""
import numpy as np
import torch

# the largest row tile of the kernels under test is 256 rows (the convolution's pair tiles / chunk granule); the pooling kernels get
# their largest block height (rows_per_block <= 128) on top, so that a store one whole tile too far still lands in the guard
GUARD_ROWS = 256 + 128
GUARD_ELEMS = 4096             # the 1-D form: elements (a multiple of 16, so every dtype keeps its 16-byte alignment)

INT_VIEW = {torch.float32: torch.int32, torch.float16: torch.int16, torch.int32: torch.int32, torch.int64: torch.int64,
            torch.uint8: torch.uint8}


def _signed(v, bits):
    return v - (1 << bits) if v >= 1 << (bits - 1) else v


# quiet NaNs with a marked payload (f32: exponent 0xFF + bit 22, f16: exponent 0x1F + bit 9); constants no kernel produces for the
# index types (negative, far outside any row count); 0xA5 / 0x5A bytes
POISON = {
    "out": {torch.float32: 0x7FC5A5A5, torch.float16: 0x7EA5, torch.int32: _signed(0xA5A5A5A5, 32),
            torch.int64: _signed(0xA5A5A5A5A5A5A5A5, 64), torch.uint8: 0xA5},
    "in": {torch.float32: 0x7FD3C3C3, torch.float16: 0x7F3C, torch.int32: _signed(0xC3C3C3C3, 32),
           torch.int64: _signed(0xC3C3C3C3C3C3C3C3, 64), torch.uint8: 0x5A},
}


class Fence:
    def __init__(self, buf, rows, cols, pitch, guard, kind):
        self.buf, self.rows, self.cols, self.pitch, self.guard, self.kind = buf, rows, cols, pitch, guard, kind
        self.dtype = buf.dtype
        self.poison = POISON[kind][buf.dtype]

    def ints(self):
        """the whole allocation as integers: [guard + rows + guard, pitch] (2-D form) or [guard + rows + guard] (1-D form)"""
        v = self.buf.view(INT_VIEW[self.dtype])
        return v if self.cols is None else v.view(-1, self.pitch)

    def changed(self):
        """(row, column) of the first changed guard element relative to the view (rows before it are negative, the 1-D form
        reports column 0), or None"""
        bad = self.ints() != self.poison
        g = self.guard
        if self.cols is None:
            bad[g:g + self.rows] = False
        else:
            bad[g:g + self.rows, :self.cols] = False
        if not bool(bad.any()):
            return None
        first = int(bad.reshape(-1).nonzero()[0, 0])
        if self.cols is None:
            return first - g, 0
        return first // self.pitch - g, first % self.pitch

    def changed_rows(self):
        """the set of rows (relative to the view) that hold a changed guard element"""
        bad = self.ints() != self.poison
        g = self.guard
        if self.cols is None:
            bad[g:g + self.rows] = False
            return sorted({int(i) - g for i in bad.nonzero()[:, 0].tolist()})
        bad[g:g + self.rows, :self.cols] = False
        return sorted({int(i) - g for i in bad.any(dim=1).nonzero()[:, 0].tolist()})


def fenced(rows, cols, dtype, pitch=None, guard_rows=None, kind="out", device="cpu"):
    """A view of `rows` x `cols` (row stride `pitch`, default cols) -- or of `rows` elements when cols is None -- with guard_rows
    poisoned rows (elements in the 1-D form) before and after it and poisoned pitch columns, all in one allocation.  The view itself
    starts as poison too (an output that must be written whole is checked with `unwritten`).  The view is 16-byte aligned: the pitch
    must be a multiple of 16 bytes, as the kernels demand.  The fence travels with the view as its attribute `fence`."""
    if kind not in POISON:
        raise ValueError(f"fenced: kind={kind!r}")
    if dtype not in INT_VIEW:
        raise ValueError(f"fenced: no poison for {dtype}")
    item = torch.empty((), dtype=dtype).element_size()
    if cols is None:
        if pitch is not None:
            raise ValueError("fenced: the 1-D form has no pitch")
        g = GUARD_ELEMS if guard_rows is None else int(guard_rows)
        if g * item % 16:
            raise ValueError(f"fenced: {g} guard elements of {dtype} break the 16-byte alignment")
        total, p = g + rows + g, 1
    else:
        p = cols if pitch is None else int(pitch)
        g = GUARD_ROWS if guard_rows is None else int(guard_rows)
        if p < cols or p * item % 16:
            raise ValueError(f"fenced: pitch {p} of {dtype} must be >= {cols} columns and a multiple of 16 bytes")
        total = (g + rows + g) * p
    poison = POISON[kind][dtype]
    buf = torch.full((total,), poison, dtype=INT_VIEW[dtype], device=device).view(dtype)
    if cols is None:
        view = buf.as_strided((rows,), (1,), g)
    else:
        view = buf.as_strided((rows, cols), (p, 1), g * p)
    assert view.data_ptr() % 16 == 0
    view.fence = Fence(buf, rows, cols, p, g, kind)
    return view


def fence_in(t, pitch=None, guard_rows=None):
    """An input fence holding the values of t (1-D or 2-D), on t's device"""
    if t.dim() == 1:
        v = fenced(t.shape[0], None, t.dtype, guard_rows=guard_rows, kind="in", device=t.device)
    else:
        v = fenced(t.shape[0], t.shape[1], t.dtype, pitch=pitch, guard_rows=guard_rows, kind="in", device=t.device)
    v.copy_(t)
    return v


def _fence(f):
    return f if isinstance(f, Fence) else f.fence


def assert_intact(*fences):
    """Every guard element of every fence still holds its poison; else the first changed one is named, relative to the view."""
    for i, f in enumerate(fences):
        f = _fence(f)
        at = f.changed()
        if at is not None:
            r, c = at
            got = int(f.ints().reshape(-1)[(r + f.guard) * f.pitch + c])
            raise AssertionError(f"fence {getattr(f, 'name', i)} ({f.kind}, {f.dtype}, view {f.rows} x {f.cols}, pitch {f.pitch}): guard element changed at "
                                 f"(row {r}, column {c}): {got & ((1 << 64) - 1):#x} instead of {f.poison & ((1 << 64) - 1):#x}")


def unwritten(t):
    """Number of elements that still hold the poison an output starts with -- a fenced view's own, or the output poison of a plain
    tensor filled with it (an output that must be written whole: 0)"""
    f = getattr(t, "fence", None)
    return int((t.view(INT_VIEW[t.dtype]) == (f.poison if f is not None else POISON["out"][t.dtype])).sum())


# ------------------------------------------------------------------------------------------ the two runs of a case
class Arena:
    """Hands a case its arrays: plain ones (contiguous, exactly sized; outputs start as the poison too, so what a kernel leaves
    unwritten compares equal) or fenced ones.  pitch=None: an array the ABI takes without a leading dimension -- one flat fence
    around all of it."""

    def __init__(self, fence):
        self.fence, self.fences = fence, []

    def _keep(self, v, name):
        v.fence.name = name or f"#{len(self.fences)}"
        self.fences.append(v.fence)

    def inp(self, t, pitch=None, name=None):
        t = t.cuda()
        if not self.fence:
            return t.contiguous().clone()
        if pitch is None or t.dim() == 1:
            v = fence_in(t.contiguous().reshape(-1))
            self._keep(v, name)
            return v.view(t.shape)
        v = fence_in(t, pitch)
        self._keep(v, name)
        return v

    def out(self, shape, dtype, pitch=None, name=None):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        if not self.fence:
            return torch.full(shape, POISON["out"][dtype], dtype=INT_VIEW[dtype], device="cuda").view(dtype)
        if pitch is None or len(shape) == 1:
            v = fenced(int(np.prod(shape)), None, dtype, device="cuda")
            self._keep(v, name)
            return v.view(shape)
        v = fenced(shape[0], shape[1], dtype, pitch=pitch, device="cuda")
        self._keep(v, name)
        return v


def bits(t):
    return t.contiguous().view(INT_VIEW[t.dtype])


def run(case):
    """case(arena) -> {name: output tensor}.  Runs it plain and fenced; the fences must be intact and the outputs the same bits.
    Returns the plain run's outputs."""
    got = []
    for fence in (False, True):
        a = Arena(fence)
        outs = case(a)
        torch.cuda.synchronize()
        assert_intact(*a.fences)
        got.append({k: v.clone() for k, v in outs.items()})
    for k in got[0]:
        x, y = bits(got[0][k]), bits(got[1][k])
        assert x.shape == y.shape, k
        if not torch.equal(x, y):
            at = (x != y).nonzero()[0].tolist()
            raise AssertionError(f"{k}: the fenced call differs from the plain call, first at {at}: {got[1][k][tuple(at)].item()} "
                                 f"instead of {got[0][k][tuple(at)].item()} ({int((x != y).sum())} elements)")
    return got[0]
