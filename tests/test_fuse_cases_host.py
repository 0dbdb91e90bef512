"""The cases of tests/fuse_cases.py hold what they claim (CPU only): chunk sizes, distinct keys, the threshold key's top byte at the
first and the last radix digit, the entry with nothing seen, the gap, and the value edges of the fp32 -> fp16 conversion."""
import numpy as np
import pytest
import torch

import fuse_cases as fc


def test_fmix32_is_murmur3s_finaliser_and_a_bijection_on_a_sample():
    # fmix32(0) = 0 and the published avalanche of 1
    assert int(fc.fmix32(0)) == 0 and int(fc.fmix32(1)) == 0x514E28B7
    x = np.arange(1 << 16, dtype=np.uint64) * np.uint64(65521)
    assert len(np.unique(fc.fmix32(x))) == len(x)


@pytest.mark.parametrize("name", fc.CASES)
def test_chunks_have_exactly_min_n_split_members_and_distinct_keys(name):
    c = fc.case(name)
    for b in range(c.B):
        n = len(c.rows_of(b))
        for k in range(c.num_files):
            h = fc.keys(c.seed, b, k, n)
            assert len(np.unique(h)) == n and (n == 0 or int(h.max()) < 2 ** 32)
            ch = fc.chunk(c.seed, b, k, n, c.n_split)
            assert int(ch.sum()) == (n if c.n_split is None else min(n, c.n_split))
            if c.n_split is not None and n > c.n_split:
                assert np.array_equal(ch, h <= fc.threshold(c.seed, b, k, n, c.n_split))


def test_selection_cases_cover_the_sizes_the_issue_names():
    c = fc.case(fc.SELECTION[0])
    assert {b: len(c.rows_of(b)) for b in range(c.B) if len(c.rows_of(b))} == fc.SIZES
    assert sorted(fc.SIZES.values())[:7] == [1, 63, 64, 65, 257, 300, 1025] and fc.SIZES[fc.LARGEST] == 2500
    assert len(c.rows_of(fc.GAP_ENTRY)) == 0 and not c.seen[c.rows_of(fc.UNSEEN_ENTRY)].any() and c.seen.any()
    # the rows of different entries interleave
    assert (np.diff(c.batch) != 0).sum() > c.N // 2
    assert {fc.case(n).n_split for n in fc.SELECTION} == {1, 64, 2499, None}
    assert {fc.case(n).num_files for n in fc.SELECTION} == {1, 3} and {fc.case(n).seed for n in fc.SELECTION} == {0, 1, 2 ** 63 + 5}


@pytest.mark.parametrize("name", fc.TOP_BYTE_00 + fc.TOP_BYTE_FF)
def test_threshold_top_byte_is_the_first_or_the_last_digit(name):
    c = fc.case(name)
    n = fc.SIZES[fc.LARGEST]
    want = 0x00 if name in fc.TOP_BYTE_00 else 0xFF
    assert c.n_split == (1 if want == 0 else n - 1)
    for k in range(c.num_files):
        assert fc.threshold(c.seed, fc.LARGEST, k, n, c.n_split) >> 24 == want, (name, k)


@pytest.mark.parametrize("name", fc.SELECTION)
def test_the_unseen_entry_and_the_gap(name):
    c = fc.case(name)
    merged, chunk = fc.reference(name, "merged"), fc.reference(name, "chunk")
    n = fc.SIZES[fc.UNSEEN_ENTRY]
    for k in range(c.num_files):
        for ref, rows in ((merged, 0), (chunk, n if c.n_split is None else min(n, c.n_split))):
            assert ref.offsets[k, fc.UNSEEN_ENTRY + 1] - ref.offsets[k, fc.UNSEEN_ENTRY] == rows
            assert ref.files[(fc.UNSEEN_ENTRY, k)]["feat"].shape == (rows, c.D)
            assert ref.offsets[k, fc.GAP_ENTRY + 1] == ref.offsets[k, fc.GAP_ENTRY]
        assert not chunk.files[(fc.UNSEEN_ENTRY, k)]["mask"].any()
    assert merged.mask is None and chunk.mask.shape == (chunk.feat.shape[0],)
    assert merged.feat.shape[0] == merged.offsets[-1, -1] == merged.mask_full.sum() and chunk.feat.shape[0] == chunk.mask_full.sum()


def test_files_differ_and_rows_go_to_different_subsets_of_files():
    c, ref = fc.case("sel_64_f3_s0"), fc.reference("sel_64_f3_s0", "chunk")
    per_row = ref.mask_full[:, c.rows_of(fc.LARGEST)].sum(0)
    assert set(np.unique(per_row)) >= {0, 1} and not np.array_equal(ref.mask_full[0], ref.mask_full[1])
    w = fc.reference("d8", "chunk").mask_full[:, fc.case("d8").rows_of(0)].sum(0)
    assert set(np.unique(w)) >= {0, 1, 2}                      # 64 of 130, three files: none, one and several files per row


def test_width_cases_cover_every_access_path_and_end_in_a_file_of_one_row():
    assert set(fc.WIDTHS) >= {1, 3, 4, 8, 12, 64, 260, 512, 520}
    assert {d % 8 == 0 for d in fc.WIDTHS} == {True, False} and any(d % 4 == 0 and d % 8 for d in fc.WIDTHS) and any(d % 4 == 2 for d in fc.WIDTHS)
    for form in fc.FORMS:
        ref = fc.reference("d1", form)
        assert ref.offsets[-1, -1] - ref.offsets[-1, -2] == 1
    assert fc.case("misaligned_d8").misaligned and fc.case("half_in_d8").features.dtype == torch.float16
    assert fc.case("f32_out_d8").dtype == torch.float32


def test_value_case_holds_the_conversion_edges():
    c, ref = fc.case("values"), fc.reference("values", "merged")
    assert np.array_equal(ref.rows, np.concatenate([c.rows_of(0), c.rows_of(1)]))
    src = c.features[torch.from_numpy(ref.rows)].reshape(-1)
    got = ref.feat.reshape(-1)
    assert got.dtype == torch.float16

    def out_of(v):
        at = (src.view(torch.int32) == torch.tensor(v, dtype=torch.float32).view(torch.int32)).nonzero()
        assert at.numel(), v
        return got[at[0, 0]]

    assert out_of(65504.0) == 65504 and out_of(65519.996) == 65504 and torch.isinf(out_of(65520.0)) and torch.isinf(out_of(-65520.0))
    assert out_of(1.0 + 2.0 ** -11) == 1.0 and out_of(1.0 + 3 * 2.0 ** -11).item() == 1.0 + 2.0 ** -9     # ties to even, both ways
    assert out_of(6e-8).view(torch.int16) == 1 and out_of(2.0 ** -25).view(torch.int16) == 0 and out_of(2.98e-8).view(torch.int16) == 0
    assert 0 < out_of(1e-6).item() < 2.0 ** -14                                                       # a half subnormal, kept
    assert out_of(-0.0).view(torch.int16).item() == -32768 and out_of(1e30) == float("inf") and out_of(-1e-30).view(torch.int16).item() == -32768
    assert torch.isnan(src).sum() == 2 and torch.equal(torch.isnan(got), torch.isnan(src))
