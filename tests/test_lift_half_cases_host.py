"""The cases of tests/lift_half_cases.py are what they claim to be (CPU only): every half case's maps and mask logits are representable in
their dtype, the oracle reference is the one of the rounded values, the conversion case holds the values it names and one point per
pixel, the alignment helper really yields a base address that is 2 mod 4, the widths meet every vector form, and the mixed streams
hold a chunk of one view and all three kinds."""
import numpy as np
import pytest
import torch

import lift_batched_cases as lb
import lift_half_cases as lh
import lift_masks_batched_cases as lm

KEYS = tuple(lh.DTYPES)


@pytest.mark.parametrize("key", KEYS)
def test_lift_cases_are_representable_and_keep_their_geometry(key):
    dtype = lh.DTYPES[key]
    for name in lh.LIFT_CASES + lh.WIDTH_CASES:
        c, base = lh.case(name, key), lh.base_case(name)
        assert c.maps.dtype == np.float32 and lh.representable(c.maps, dtype), name
        half = torch.from_numpy(c.maps).to(dtype)
        assert np.array_equal(half.float().numpy().view(np.int32), c.maps.view(np.int32)), name
        assert np.abs(c.maps).max() <= 1.0                                       # (the bilinear tolerance of the GPU tests is stated for maps in [-1, 1])
        # rounding moved a value by at most half an ulp of the dtype at 1, and moved some (the rounded case is not the fp32 case)
        err = np.abs(c.maps.astype(np.float64) - base.maps)
        assert err.max() <= (2.0 ** -11 if key == "fp16" else 2.0 ** -8) * 0.5 * 2 and (c.maps.size < 64 or err.max() > 0), name
        for f in ("points", "view_entry", "w2c", "intr"):
            assert np.array_equal(getattr(c, f), getattr(base, f)), (name, f)
        assert (c.mode, c.cut, c.tau, c.min_visible, c.max_visible, c.H, c.W) == (base.mode, base.cut, base.tau, base.min_visible,
                                                                                  base.max_visible, base.H, base.W)
        assert c.H <= 12 and c.W <= 16


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("name", ["D65", "views_130_bilinear", "fill", "width_520", "width_12_bilinear"])
def test_the_reference_is_the_oracle_on_the_rounded_maps(name, key):
    c, ref = lh.case(name, key), lh.reference(name, key)
    # geometry does not depend on the maps: masks, counts and the fill's choice are the fp32 case's
    if not name.startswith("width_"):
        full = lb.reference(name)
        for f in ("seen", "count", "view_count", "view_keep", "filled_from"):
            assert np.array_equal(getattr(ref, f), getattr(full, f)), f
    # ... and the features are those of the independent restatement on the ROUNDED maps
    out = lb.restatement(c)[0]
    if c.mode == "nearest":
        assert np.array_equal(out.view(np.int32), ref.features.view(np.int32))
    else:
        assert np.abs(out - ref.features.astype(np.float64)).max() <= 1e-6
    assert ref.seen.any()


def test_the_widths_meet_every_vector_form():
    assert set(lh.WIDTHS) >= {1, 3, 8, 520, 1024}                                # the issue's list
    chunk = lb.col_chunk()
    forms = {D: lh.vector_length(D, 0) for D in lh.WIDTHS}
    assert set(forms.values()) == {1, 4, 8}
    for vec in (4, 8):                                                           # one width just below and one just above a multiple
        assert any(D % vec == vec - 1 for D in lh.WIDTHS) and any(D % vec == 1 for D in lh.WIDTHS)
    # a second pass with exactly one live lane of each vector form, two passes of the 2-byte form, two full passes
    assert forms[chunk + 8] == 8 and forms[chunk + 4] == 4 and forms[chunk + 9] == 1 and forms[2 * chunk] == 8
    # a base that is only 2-byte aligned takes the 2-byte form whatever the width
    assert all(lh.vector_length(D, 2) == 1 for D in lh.WIDTHS)
    assert lh.vector_length(8, 8) == 4 and lh.vector_length(8, 4) == 1 and lh.vector_length(12, 16) == 4


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("D", lh.CONVERSION_WIDTHS)
def test_the_conversion_case(key, D):
    c, half = lh.conversion_case(key, D)
    dtype = lh.DTYPES[key]
    assert half.dtype == dtype and half.shape == (1, D, lh.CONV_H, lh.CONV_W)
    bits = half.view(torch.int16).numpy().view(np.uint16)
    assert set(np.unique(bits).tolist()) == set(lh.CONVERSION_BITS[key])         # every named value occurs
    vals = half.float()
    assert bool(torch.isfinite(vals).all())                                      # no NaN, no inf
    fi = torch.finfo(dtype)
    named = {0.0, float(fi.smallest_normal), float(fi.max), -float(fi.max), 1.0 + float(fi.eps), -(1.0 + float(fi.eps)), -float(fi.smallest_normal)}
    sub = float(fi.smallest_normal) * float(fi.eps)                              # the smallest subnormal
    named |= {sub, -sub, float(fi.smallest_normal) - sub, -(float(fi.smallest_normal) - sub)}
    assert set(vals.unique().tolist()) == named
    assert bool((vals == 0).any()) and bool((torch.signbit(vals) & (vals == 0)).any())   # both zeros
    # one point per pixel, each exactly on its pixel and visible; a count of 1 everywhere
    ref = lb._reference(c)
    assert ref.seen.all() and (ref.count == 1).all() and ref.view_count.tolist() == [lh.CONV_H * lh.CONV_W]
    rows, x, y = ref.lists[0]
    assert np.array_equal(rows, np.arange(c.N)) and np.array_equal(x * lh.CONV_W + y, np.arange(c.N))
    expected, conv = lh.conversion_expected(key, D)
    assert expected.dtype == np.float32 and expected.shape == (c.N, D)
    # the expectation is the converted value bit for bit, except that -0 comes out of the sum as +0
    same = expected.view(np.int32) == conv.view(np.int32)
    assert (same | (conv.view(np.int32) == np.int32(-2 ** 31))).all() and not same.all()
    assert np.array_equal(expected.view(np.int32), ref.features.view(np.int32))  # ... and the oracle's lift says the same
    # every named value meets every position inside a group of `vec` channels
    vec = lh.vector_length(D, 0)
    per_pixel = bits.reshape(D, -1).T
    for i in range(vec):
        assert set(np.unique(per_pixel[:, i::vec]).tolist()) == set(lh.CONVERSION_BITS[key]), i


@pytest.mark.parametrize("key", KEYS)
def test_the_alignment_helper_yields_a_base_of_2_mod_4(key):
    dtype = lh.DTYPES[key]
    for name in lh.ALIGNMENT_CASES:
        c = lh.case(name, key)
        t = torch.from_numpy(c.maps).to(dtype)
        for layout in ("nchw", "channels_last"):
            src = t if layout == "nchw" else t.contiguous(memory_format=torch.channels_last)
            v = lh.misaligned(src)
            assert v.data_ptr() % 4 == 2 and v.shape == t.shape and torch.equal(v.view(torch.int16), t.view(torch.int16))
            assert v.is_contiguous() if layout == "nchw" else v.is_contiguous(memory_format=torch.channels_last)
            assert lh.vector_length(c.D, v.data_ptr()) == 1
    assert {lh.case(n, key).D % 2 for n in lh.ALIGNMENT_CASES} == {0, 1}
    assert {lh.case(n, key).mode for n in lh.ALIGNMENT_CASES} == {"nearest", "bilinear"}


def test_the_mixed_streams():
    for name in lh.STREAM_CASES:
        c, chunks = lh.stream_case(name)
        assert np.array_equal(np.concatenate([idx for idx, _ in chunks]), np.arange(c.V))
        assert {k for _, k in chunks} == set(lh.STREAM_KINDS) and any(len(idx) == 1 for idx, _ in chunks)
        for idx, kind in chunks:
            assert kind == "fp32" or lh.representable(c.maps[idx], lh.DTYPES[kind]), (name, kind)
        assert not lh.representable(c.maps, torch.float16) or c.maps.size < 64   # (the fp32 chunk stayed fp32)
    for name in lh.MASK_CASES:
        c, chunks = lh.mask_stream_case(name)
        assert np.array_equal(np.concatenate([idx for idx, _ in chunks]), np.arange(c.V))
        assert any(len(idx) == 1 for idx, _ in chunks) and (c.V < 3 or any(len(idx) > 1 for idx, _ in chunks))
        for idx, kind in chunks:
            assert kind == "fp32" or lh.representable(c.pred_masks[idx], lh.DTYPES[kind]), (name, kind)


@pytest.mark.parametrize("key", KEYS)
def test_the_mask_cases(key):
    dtype = lh.DTYPES[key]
    qs = set()
    for name in lh.MASK_CASES:
        c = lh.mask_case(name, key)
        assert lh.representable(c.pred_masks, dtype), name
        assert c.H <= 12 and c.W <= 16 and c.h <= 8 and c.w <= 10
        qs.add(c.Q)
    assert {1, 64, 65} <= qs and max(qs) == max(lm.case(n).Q for n in lm.CASES)
    z = lh.mask_case("zero_logit", key)
    block = z.pred_masks[:, :, lh.ZERO_BLOCK[0], lh.ZERO_BLOCK[1]]
    assert block.size and (block == 0).all() and (z.h, z.w) == (z.H, z.W)        # logits of exactly 0 that the resize leaves alone
    assert (np.abs(z.pred_masks) > 0).any()
