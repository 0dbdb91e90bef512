"""Cases for the four batched lifts on fp16 / bf16 inputs (sparse.lift, LiftStream, lift_masks, LiftMasksStream reading half maps and half
mask logits in place).  numpy / torch on the CPU, no device code.  Nothing here edits the case libraries it builds on.

A half case is a case of tests/lift_batched_cases.py or tests/lift_masks_batched_cases.py whose maps (mask logits) were rounded to the
half dtype and converted back: the fp32 arrays of the case then hold values the dtype represents, `x.to(dtype).float() == x`, so the
half tensor and its fp32 copy are the same numbers and the yardstick of the GPU tests is exact: the call on the half tensor gives the
bits of the call on the fp32 copy.  The oracle reference of a half case is lift_batched_cases' own reference computed on the rounded
values.

Widths.  The lift kernels take 8 consecutive channels of a half row with one 16-byte load when D % 8 == 0 and the maps' base address is
16-byte aligned, 4 with one 8-byte load when D % 4 == 0 and the base is 8-byte aligned, and one 2-byte element otherwise; a pass holds
512 channels.  WIDTHS covers: 1 and 3 (below both vector lengths), 5 (just above 4), 7 and 9 (just below and above 8), 8 and 12 (the
16- and the 8-byte form), 516 and 520 (a second pass with one live lane of the 8- and the 16-byte form), 521 (two passes of the
2-byte form) and 1024 (two full passes).

The conversion case holds, for each dtype, the values a wrong conversion would lose: +-0, the smallest and the largest subnormal, the
smallest normal, 1 + one ulp and +- the largest finite value, as bit patterns; one entry, one identity view, one point on every
pixel, so a row of the result is one map column: (+0) + x, divided by a count of 1.
"""
import numpy as np
import torch

import lift_batched_cases as lb
import lift_masks_batched_cases as lm

f32, f64 = np.float32, np.float64
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
LIFT_CASES = ("views_130", "views_130_bilinear", "D65", "D_chunk_plus_1", "D_chunk_plus_1_bilinear", "bilinear_h1", "entries", "twins", "fill", "drop")
WIDTHS = (1, 3, 5, 7, 8, 9, 12, 516, 520, 521, 1024)
MASK_CASES = ("Q1", "Q64", "Q65", "Q1024", "views_0_1_63", "twins", "fill_inview", "zero_logit")
VEC_BYTES = {8: 16, 4: 8, 1: 2}                             # channels a lane takes with one load -> the alignment the rows need


def rounded(a, dtype):
    """the fp32 array a rounded to dtype (round to nearest even, torch's conversion) and back: values the dtype holds"""
    return torch.from_numpy(np.ascontiguousarray(a, f32)).to(dtype).float().numpy()


def representable(a, dtype):
    t = torch.from_numpy(np.ascontiguousarray(a, f32))
    return bool(torch.equal(t.to(dtype).float().view(torch.int32), t.view(torch.int32)))


def vector_length(D, base_address):
    """the channels a lane takes with one load from half maps of D channels whose first element lies at base_address"""
    for vec in (8, 4):
        if D % vec == 0 and base_address % VEC_BYTES[vec] == 0:
            return vec
    return 1


# ------------------------------------------------------------------------------------------ the dense lift
def _width_case(D, bilinear):
    if bilinear:
        return lb.generic(f"width_{D}_bilinear", 300 + D, {0: 40, 1: 30}, {0: 3, 1: 2}, D, hw=(3, 4), image_shape=(6, 8), mode="bilinear")
    return lb.generic(f"width_{D}", 100 + D, {0: 40, 1: 30}, {0: 3, 1: 2}, D, hw=(6, 8))


WIDTH_CASES = tuple(f"width_{D}" for D in WIDTHS) + tuple(f"width_{D}_bilinear" for D in WIDTHS)
_BASE, _HALF, _REFERENCES = {}, {}, {}


def base_case(name):
    """the fp32 case a half case is rounded from: a library case, or one of the width cases"""
    if name not in _BASE:
        if name.startswith("width_"):
            parts = name.split("_")
            _BASE[name] = _width_case(int(parts[1]), len(parts) == 3)
        else:
            _BASE[name] = lb.case(name)
    return _BASE[name]


def with_maps(c, maps, name=None):
    """the lift_batched_cases.Case c with other maps (same geometry, options and notes)"""
    return lb.Case(name or c.name, c.points, maps, c.view_entry, c.w2c, c.intr, c.depth, (c.H, c.W), c.mode, c.cut, c.tau, c.min_visible,
                   c.max_visible, **c.notes)


def case(name, key):
    """the case `name` with its maps rounded to DTYPES[key]; computed once and shared: callers must not change it"""
    if (name, key) not in _HALF:
        c = base_case(name)
        _HALF[name, key] = with_maps(c, rounded(c.maps, DTYPES[key]))
    return _HALF[name, key]


def reference(name, key):
    """the oracle reference of tests/lift_batched_cases.py on the rounded maps; computed once and shared"""
    if (name, key) not in _REFERENCES:
        _REFERENCES[name, key] = lb._reference(case(name, key))
    return _REFERENCES[name, key]


# ------------------------------------------------------------------------------------------ exact conversion
CONVERSION_BITS = {
    # +0, -0, smallest subnormal, largest subnormal, smallest normal, 1 + ulp, largest finite, and the negative of each but the zeros
    "fp16": (0x0000, 0x8000, 0x0001, 0x03FF, 0x0400, 0x3C01, 0x7BFF, 0x8001, 0x83FF, 0x8400, 0xBC01, 0xFBFF),
    "bf16": (0x0000, 0x8000, 0x0001, 0x007F, 0x0080, 0x3F81, 0x7F7F, 0x8001, 0x807F, 0x8080, 0xBF81, 0xFF7F),
}
CONVERSION_WIDTHS = (8, 12, 3)                              # the 16-byte, the 8-byte and the 2-byte form
CONV_W, CONV_H, CONV_FX = 16, 12, 8.0


def conversion_bits(key, D):
    """int16 [1, D, H, W]: the bit patterns of CONVERSION_BITS[key] in turn over the map's elements (every value meets every lane
    position of a vector load: 12 values against groups of 8, 4 or 1 channels over 192 pixels)"""
    pat = np.array(CONVERSION_BITS[key], np.uint16)
    n = D * CONV_H * CONV_W
    flat = pat[(np.arange(n) % D + np.arange(n) // D) % len(pat)]               # (channel + pixel) mod 12
    return flat.reshape(1, CONV_H, CONV_W, D).transpose(0, 3, 1, 2).copy().view(np.int16)


def conversion_case(key, D):
    """-> (lift_batched_cases.Case on the converted values, the half maps as a torch tensor [1,D,H,W] of DTYPES[key]).  Point p = row *
    W + col of the one entry projects exactly onto pixel (row, col): identity camera, focal 8, centre (8, 6), z = 1, dyadic x and y."""
    bits = conversion_bits(key, D)
    half = torch.from_numpy(bits).view(DTYPES[key])
    col, row = np.meshgrid(np.arange(CONV_W), np.arange(CONV_H))
    pts = np.column_stack([np.zeros(CONV_W * CONV_H), (col.reshape(-1) - 8) / 8.0, (row.reshape(-1) - 6) / 8.0, np.ones(CONV_W * CONV_H)])
    M, K = lb._identity_views(1, CONV_FX, CONV_W, CONV_H)
    return lb.Case(f"conversion_{key}_{D}", pts, half.float().numpy(), [0], M, K, None), half


def conversion_expected(key, D):
    """fp32 [H*W, D]: what the lift returns for conversion_case -- row p is the map column of pixel p converted on the CPU and added to
    the +0 the sum starts from ((+0) + (-0) = +0 in round to nearest: the one value whose bits the sum changes), divided by 1"""
    _, half = conversion_case(key, D)
    conv = half.float().numpy()[0].transpose(1, 2, 0).reshape(CONV_H * CONV_W, D)
    return (f32(0) + conv) / f32(1), conv


# ------------------------------------------------------------------------------------------ alignment
def misaligned(t):
    """a tensor of t's shape, dtype, device and values that is a view into a flat buffer starting at element 1: for a 2-byte dtype its
    base address is 2 mod 4.  A channels_last t stays channels_last, a contiguous one contiguous."""
    assert t.element_size() == 2 and t.dim() == 4
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    assert flat.data_ptr() % 16 == 0
    if t.is_contiguous():
        v = flat[1:].view(t.shape)
    else:
        assert t.is_contiguous(memory_format=torch.channels_last)
        V, D, h, w = t.shape
        v = flat[1:].view(V, h, w, D).permute(0, 3, 1, 2)
    v.copy_(t)
    assert v.data_ptr() % 4 == 2
    return v


ALIGNMENT_CASES = ("width_8", "width_9", "width_12_bilinear", "width_521_bilinear", "D65")   # D even and odd, both modes


# ------------------------------------------------------------------------------------------ streams of mixed dtypes
STREAM_CASES = ("views_130_bilinear", "D_chunk_plus_1", "twins", "width_520")
STREAM_KINDS = ("fp16", "fp32", "bf16")


def stream_chunks(c):
    """[(view indices, kind)]: consecutive slices of the views in the kinds fp16, fp32, bf16 in turn -- a chunk of one view first, then
    chunks of 2, 1 and the rest"""
    sizes = [1, 2, 1]
    cuts = np.cumsum([0] + [s for s in sizes if s < c.V])
    cuts = [int(x) for x in cuts if x < c.V] + [c.V]
    return [(np.arange(a, b), STREAM_KINDS[i % 3]) for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:]))]


def stream_case(name):
    """-> (the case with every chunk's maps rounded to the chunk's kind, the chunks)"""
    if ("stream", name) not in _HALF:
        c = base_case(name)
        chunks = stream_chunks(c)
        maps = c.maps.copy()
        for idx, kind in chunks:
            if kind != "fp32":
                maps[idx] = rounded(maps[idx], DTYPES[kind])
        _HALF["stream", name] = (with_maps(c, maps), chunks)
    return _HALF["stream", name]


# ------------------------------------------------------------------------------------------ masks
ZERO_BLOCK = (slice(2, 6), slice(3, 7))                     # pixel rows and columns of "zero_logit" whose logits are exactly 0


def _mask_base(name):
    if name != "zero_logit":
        return lm.case(name)
    # masks of the image's own size: the resize is the identity (taps 0, 1, 0, 0), a logit of exactly 0 stays 0 and sigmoid(0) = 0.5
    # sits on the threshold of "the query keeps its pixel"
    c = lm.case("mask_full")
    pm = c.pred_masks.copy()
    pm[:, :, ZERO_BLOCK[0], ZERO_BLOCK[1]] = 0.0
    return lm.Case("zero_logit", c.geo, pm, c.pred_logits, c.mask_embed, c.text, c.scale)


def mask_case(name, key):
    """the mask case `name` with pred_masks rounded to DTYPES[key] ("fp32": as they are); computed once and shared"""
    if ("mask", name, key) not in _HALF:
        c = _mask_base(name)
        pm = c.pred_masks if key == "fp32" else rounded(c.pred_masks, DTYPES[key])
        _HALF["mask", name, key] = lm.Case(name, c.geo, pm, c.pred_logits, c.mask_embed, c.text, c.scale, exact=c.exact, **c.notes)
    return _HALF["mask", name, key]


def mask_chunks(c):
    """[(view indices, kind)] for LiftMasksStream: a chunk of one view, then chunks of several, the kinds fp16, fp32, bf16 in turn"""
    return stream_chunks(c)


def mask_stream_case(name):
    """-> (the case with every chunk's pred_masks rounded to the chunk's kind, the chunks)"""
    if ("mask_stream", name) not in _HALF:
        c = _mask_base(name)
        chunks = mask_chunks(c)
        pm = c.pred_masks.copy()
        for idx, kind in chunks:
            if kind != "fp32":
                pm[idx] = rounded(pm[idx], DTYPES[kind])
        _HALF["mask_stream", name] = (lm.Case(name, c.geo, pm, c.pred_logits, c.mask_embed, c.text, c.scale, exact=c.exact, **c.notes), chunks)
    return _HALF["mask_stream", name]
