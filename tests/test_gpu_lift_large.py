"""The lifts over batched point clouds past the sizes at which their shared kernels change behaviour (csrc/gp_lift_entries.h,
gp_lift_stream_state.h, lift_masks_batched.hip): more than one block of 256 fill queries, more than one LDS trip of 1024 references,
a block whose range is the union of several entries' runs, a second trip of the count kernels' stride loop and of the ordered walk
(an entry of more than 16 384 rows), and rows beyond the 65 538 words of the offset table.  The cases are lift_batched_cases.LARGE
(fill_blocks, fill_tie_trips, walk_trips, rows_past_table); tests/test_lift_batched_cases_host.py asserts on the CPU, from the
references, that each of them reaches what it is named for.  sparse.lift, sparse.LiftStream, the visible lists of the mask lift,
sparse.lift_masks, sparse.LiftMasksStream, sparse.lift_labels and its stream all run them.

Bounds: those of the files whose rules are imported.  Exact -- seen, count, view_count, view_keep, the fill's choice (nn), the status
words, the visible lists, labels and votes, and the "nearest" features bit for bit (tests/test_gpu_lift_batched.py); a stream equals
the one call bit for bit (tests/test_gpu_lift_stream.py, tests/test_gpu_lift_masks_stream.py); the mask lift's features within TOL_LIFT
= 1e-5 of the reference off the rows the reference's own near-tie flags cover (tests/test_gpu_lift_masks_batched.py), which
tests/test_lift_masks_batched_cases_host.py caps at 1 % of a case's rows.

The helpers are the ones of those files, imported: one rule, stated once.  The references are computed once per module and process
(reference() of the case modules) and never changed.
"""
import numpy as np
import pytest
import torch

import lift_batched_cases as lb
import lift_labels_cases as ll
import lift_masks_batched_cases as lm
import lift_stream_cases as ls
import test_gpu_lift_batched as tb
import test_gpu_lift_labels as tl
import test_gpu_lift_masks_batched as tm
import test_gpu_lift_masks_stream as tms
import test_gpu_lift_stream as ts

pytestmark = pytest.mark.gpu

STREAMED = ("fill_blocks", "walk_trips", "rows_past_table")
KINDS = ("whole", "split")


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from geopurify_amd import _lib, ops, sparse
    _lib.load()
    return ops, sparse


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _chunks(c, kind):
    """"whole": one chunk.  "split": two chunks of consecutive views, cut inside the views of the entry that has the most of them (entry 1
    of walk_trips: one view before the cut, two after it; entry 0 of fill_blocks; entry 2 of rows_past_table) -- the concatenation is
    the case's own view order, so the reference is the case's"""
    if kind == "whole":
        return ls.partition(c, "whole")
    vs = c.views_of(ls.widest_entry(c))
    assert len(vs) >= 2
    cut = int(vs[len(vs) // 2])
    chunks = [np.arange(cut, dtype=np.int64), np.arange(cut, c.V, dtype=np.int64)]
    assert all(len(np.intersect1d(ch, vs)) for ch in chunks)
    return chunks


# ------------------------------------------------------------------------------------------ the dense lift
@pytest.mark.parametrize("name", lb.LARGE)
def test_lift_matches_the_reference(env, name):
    """sparse.lift and ops.lift_batched: the rule of tests/test_gpu_lift_batched.py::test_lift_matches_the_reference, all of it exact"""
    c, ref = lb.case(name), lb.reference(name)
    assert c.mode == "nearest"
    got = tb._lift(env, c)
    assert got.features.dtype == torch.float32 and got.features.shape == (c.N, c.D)
    assert np.array_equal(got.seen.cpu().numpy(), ref.seen) and np.array_equal(got.count.cpu().numpy(), ref.count)
    assert np.array_equal(got.view_count.cpu().numpy(), ref.view_count) and np.array_equal(got.view_keep.cpu().numpy(), ref.view_keep)
    raw = tb._raw(env, c)
    nn = raw.nn.cpu().numpy()
    wrong = np.nonzero(nn != ref.filled_from)[0]
    assert len(wrong) == 0, f"the fill's choice differs in {len(wrong)} rows, first {wrong[:5].tolist()}: {nn[wrong[:5]].tolist()} for " \
                            f"{ref.filled_from[wrong[:5]].tolist()}"
    assert raw.status.tolist()[:6] == [0, 0, 0, int(c.entries().max()), int(ref.seen.sum()), int((ref.filled_from >= 0).sum())]
    assert np.array_equal(raw.seen.cpu().numpy().astype(bool), ref.seen) and np.array_equal(raw.count.cpu().numpy(), ref.count)
    assert np.array_equal(raw.view_count.cpu().numpy(), ref.view_count) and np.array_equal(raw.view_keep.cpu().numpy().astype(bool), ref.view_keep)
    assert np.array_equal(got.features.cpu().numpy().view(np.int32), ref.features.view(np.int32))
    # without the fill an unseen row is zero and a seen row keeps its bits
    plain = tb._lift(env, c, fill=False)
    seen = got.seen
    assert torch.equal(tb._bits(plain.features[seen]), tb._bits(got.features[seen])) and not bool(plain.features[~seen].any())
    assert torch.equal(tb._bits(plain.features), tb._bits(raw.out))
    unfilled = tb._raw(env, c, fill=False)
    assert unfilled.status.tolist()[4:6] == [int(ref.seen.sum()), 0] and torch.equal(tb._bits(unfilled.out), tb._bits(raw.out))


def test_the_one_call_stays_inside_its_extents_on_fill_blocks(env):
    """ops.lift_batched on fenced arrays with eleven fill blocks, block ranges that are unions of runs and three LDS trips: the body
    of tests/test_gpu_lift_batched.py's extent test, run on the large case"""
    tb.test_the_entry_points_stay_inside_their_extents(env, "fill_blocks")


# ------------------------------------------------------------------------------------------ the dense stream
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", STREAMED)
def test_stream_matches_the_one_call_and_the_reference(env, name, kind):
    """sparse.LiftStream: ls_counts_kernel past one trip, ls_tables_kernel on both sides of the table's length, the finish's fill over
    the checked copy of the tables"""
    _, sparse = env
    c, ref = lb.case(name), lb.reference(name)
    chunks = _chunks(c, kind)
    assert np.array_equal(ls.concatenation(chunks), np.arange(c.V)) and len(chunks) == (1 if kind == "whole" else 2)
    for fill in (True, False):
        got = ts._streamed(sparse, c, chunks, fill)
        ts._assert_same(got, ts._one_call(sparse, c, np.arange(c.V), fill), f"{name} / {kind} / fill={fill}")
        if fill:
            ts._assert_reference(c, ref, got)
    st, per_chunk, fin = ts._raw(env, c, chunks)
    assert np.array_equal(fin.nn.cpu().numpy(), ref.filled_from)
    assert fin.status.tolist() == [0, 0, 0, int(c.entries().max()), int(ref.seen.sum()), int((ref.filled_from >= 0).sum()), 0, 0]
    assert np.array_equal(st.count.cpu().numpy(), ref.count)
    assert np.array_equal(torch.cat([vc for vc, _ in per_chunk]).cpu().numpy(), ref.view_count)
    assert np.array_equal(torch.cat([vk for _, vk in per_chunk]).cpu().numpy().astype(bool), ref.view_keep)


# ------------------------------------------------------------------------------------------ the visible lists of the mask lift
def _counts_only(env, c, size):
    """gp_lift_masks_batched_lists with cap = 0 and entry arrays that exist (ops.lift_masks_batched_lists passes none then): -> (the
    four entry arrays as they are afterwards, view_off, view_count, view_keep, status)"""
    ops, _ = env
    from geopurify_amd import _lib
    lib = _lib.load()
    P, ve, M, K = _dev(c.points), _dev(c.view_entry), _dev(c.w2c), _dev(c.intr)
    depth = None if c.depth is None else _dev(c.depth)
    ent = [torch.full((size,), -7, dtype=torch.int64, device="cuda") for _ in range(3)] + [torch.full((size,), -7, dtype=torch.int32, device="cuda")]
    view_off, view_count = (torch.full((k,), -7, dtype=torch.int64, device="cuda") for k in (c.V + 1, c.V))
    view_keep, status = torch.full((c.V,), 7, dtype=torch.uint8, device="cuda"), torch.full((8,), -7, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.gp_lift_masks_batched_lists_workspace_bytes(c.N, c.V), dtype=torch.uint8, device="cuda")
    ops.check(lib.gp_lift_masks_batched_lists(ops._ptr(P), c.N, ops._ptr(ve), ops._ptr(M), ops._ptr(K), ops._ptr(depth), c.V, c.H, c.W, c.cut,
                                              float(c.tau), c.min_visible, 2 ** 63 - 1 if c.max_visible is None else c.max_visible, 0,
                                              ops._ptr(ent[0]), ops._ptr(ent[1]), ops._ptr(ent[2]), ops._ptr(ent[3]), ops._ptr(view_off),
                                              ops._ptr(view_count), ops._ptr(view_keep), ops._ptr(status), ops._ptr(ws), ws.numel(), ops._stream()),
              "gp_lift_masks_batched_lists")
    torch.cuda.synchronize()
    return ent, view_off, view_count, view_keep, status


@pytest.mark.parametrize("name", ["walk_trips", "fill_blocks"])
def test_visible_lists_match_the_reference(env, name):
    """ops.lift_masks_batched_lists: lml_walk_kernel with more than one trip per part (walk_trips: 267 rows per part) and with many
    parts of one trip (fill_blocks), counting and writing"""
    c, ref = lb.case(name), lb.reference(name)
    total = int(ref.view_count.sum())
    want_off = np.concatenate([[0], np.cumsum(ref.view_count)])
    assert total == sum(len(v[0]) for v in ref.lists.values()) and total > 2000
    # cap = total (the wrapper counts, reads the total back and calls again with it)
    lists = tm._lists(env, c)
    assert lists.total == total and lists.max_views == max(len(c.views_of(b)) for b in np.unique(c.view_entry))
    assert np.array_equal(lists.view_off.cpu().numpy(), want_off) and np.array_equal(lists.view_count.cpu().numpy(), ref.view_count)
    assert np.array_equal(lists.view_keep.cpu().numpy().astype(bool), ref.view_keep)
    status = lists.status.tolist()
    assert status[:3] == [0, 0, 0] and status[3] == int(c.entries().max()) and status[5] == 0 and status[6] == total
    pt, x, y, view = (t.cpu().numpy() for t in (lists.pt, lists.x, lists.y, lists.view))
    for v in range(c.V):
        rows, px, py = ref.lists.get(v, (np.zeros(0, np.int64),) * 3)
        s = slice(int(want_off[v]), int(want_off[v + 1]))
        assert (np.diff(pt[s]) > 0).all(), v                                     # ascending by row
        assert np.array_equal(pt[s], rows) and np.array_equal(x[s], px) and np.array_equal(y[s], py) and (view[s] == v).all(), v
    # cap = 0: the counts alone, and entry arrays that exist are not touched
    ent, view_off, view_count, view_keep, st0 = _counts_only(env, c, total)
    assert all(bool((t == -7).all()) for t in ent)
    assert np.array_equal(view_off.cpu().numpy(), want_off) and np.array_equal(view_count.cpu().numpy(), ref.view_count)
    assert np.array_equal(view_keep.cpu().numpy().astype(bool), ref.view_keep)
    assert st0.tolist() == [0, 0, 0, int(c.entries().max()), 0, 0, total, lists.max_views]


# ------------------------------------------------------------------------------------------ the mask lift
@pytest.mark.parametrize("name", lm.LARGE)
def test_lift_masks_and_its_stream_match_the_reference(env, name):
    """sparse.lift_masks and sparse.LiftMasksStream (whole, and split inside an entry's views): the rule and the bound of
    tests/test_gpu_lift_masks_batched.py::test_lift_masks_matches_the_reference; the stream equals the one call bit for bit"""
    _, sparse = env
    c, ref = lm.case(name), lm.reference(name)
    got = tm._lift(env, c)
    tms._assert_reference(c, ref, got)
    lists, raw = tm._raw(env, c)
    assert np.array_equal(raw.nn.cpu().numpy(), ref.filled_from)                 # the scene-level fill's choice
    status = raw.status.tolist()
    assert status[:3] == [0, 0, 0] and status[3] == int(c.entries().max()) and status[4] == int(ref.seen.sum())
    assert status[5] == int((ref.filled_from >= 0).sum()) and status[6:] == [0, 0]
    off, seg_got = lists.view_off.tolist(), raw.seg.cpu().numpy()
    for v in range(c.V):
        rows, x, y, seg, _ = ref.views.get(v, (np.zeros(0, np.int64),) * 5)
        s = slice(off[v], off[v + 1])
        assert np.array_equal(lists.pt[s].cpu().numpy(), rows), v
        if ref.view_keep[v]:
            sure = ~ref.near[rows]
            assert np.array_equal(seg_got[s][sure], seg[sure]), v                # (the in-view fill's choice)
        else:
            assert (seg_got[s] == -1).all(), v
    plain = tm._lift(env, c, fill=False)
    seen = got.seen
    assert torch.equal(tm._bits(plain.features[seen]), tm._bits(got.features[seen])) and not bool(plain.features[~seen].any())
    for kind in KINDS:
        chunks = _chunks(c, kind)
        for fill in (True, False):
            tms._assert_same(tms._streamed(sparse, c, chunks, fill), plain if not fill else got, f"{name} / {kind} / fill={fill}")


# ------------------------------------------------------------------------------------------ the label vote
@pytest.mark.parametrize("name", ll.LARGE)
def test_lift_labels_and_its_stream_match_the_reference(env, name):
    """sparse.lift_labels and sparse.LiftLabelsStream: the fill with "voted" as its reference mask -- other runs, blocks and trips
    than the dense lift's on the same geometry (tests/test_lift_labels_cases_host.py).  Everything is an integer and exact."""
    ops, _ = env
    c, ref = ll.case(name), ll.reference(name)
    assert ref.out_of_range == 0
    got = tl._call(env, c)
    tl._assert_equal(got, ref, what=name)
    tl._assert_equal(tl._call(env, c, fill=False), ref, fill=False, what=f"{name} unfilled")
    raw = ops.lift_labels_batched(_dev(c.points), _dev(c.labels), c.C, _dev(c.view_entry), _dev(c.w2c), _dev(c.intr), tl._depth(c), c.cut, c.tau,
                                  c.min_visible, 2 ** 63 - 1 if c.max_visible is None else c.max_visible, ignore_ids=c.ignore,
                                  unlabeled=c.unlabeled)
    assert raw.status.tolist() == [0, 0, 0, int(c.entries().max()), int((ref.voted > 0).sum()), int((ref.filled_from >= 0).sum()), 0, 0]
    for kind in KINDS:
        streamed = tl._run_stream(env, c, _chunks(c, kind))
        tl._assert_equal(streamed, ref, what=f"{name} / {kind}")
        tl._assert_equal(streamed, got, what=f"{name} / {kind} against the one call")
