"""Cases for sparse.fuse / load_fused / FusedChunks.dense (csrc/fuse.hip) and the restatement of their rule.  numpy on the CPU (torch
on the CPU only for the expected rows, features[rows].to(dtype)); no device code.

The rule, restated from the issue independently of the kernels: per batch entry b, its points are the rows with batch index b in
ascending row order, local index i = 0 .. n_b - 1.  Per file k, chunk_k is all of them when n_split is None or n_b <= n_split, else
the n_split points with the smallest key
    h = fmix32(i ^ c),   c = fmix32(k ^ fmix32(b ^ fmix32(seed_lo ^ fmix32(seed_hi)))),
    fmix32(x): x ^= x >> 16; x *= 0x85ebca6b; x ^= x >> 13; x *= 0xc2b2ae35; x ^= x >> 16   (mod 2^32).
fmix32 is a bijection, so the keys of one (entry, file) are distinct and the chunk needs no tie rule.
    form "merged": mask_full = chunk_k & seen;  feat = features[mask_full].to(dtype)
    form "chunk":  mask_full = chunk_k;         feat = features[chunk_k].to(dtype);  mask = seen[chunk_k]
feat stacks the files k = 0 .. num_files - 1, inside a file the entries b = 0 .. B - 1, inside an entry ascending rows; offsets[k, b]
is where file (k, b) starts.
"""
import numpy as np
import torch

M32 = np.uint64(0xFFFFFFFF)
FORMS = ("merged", "chunk")


def fmix32(x):
    x = np.asarray(x, np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x85EBCA6B)) & M32
    x = x ^ (x >> np.uint64(13))
    x = (x * np.uint64(0xC2B2AE35)) & M32
    x = x ^ (x >> np.uint64(16))
    return x


def keys(seed, b, k, n):
    """the keys of the n points of entry b for file k, uint64 values below 2^32"""
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    c = fmix32(np.uint64(k) ^ fmix32(np.uint64(b) ^ fmix32(lo ^ fmix32(hi))))
    return fmix32(np.arange(n, dtype=np.uint64) ^ c)


def chunk(seed, b, k, n, n_split):
    """bool [n]: the local indices of chunk_k"""
    if n_split is None or n <= n_split:
        return np.ones(n, bool)
    m = np.zeros(n, bool)
    m[np.argpartition(keys(seed, b, k, n), n_split - 1)[:n_split]] = True
    return m


def threshold(seed, b, k, n, n_split):
    """the largest key inside the chunk of a selecting (entry, file)"""
    return int(np.sort(keys(seed, b, k, n))[n_split - 1])


class Case:
    """points f64 [N,4]; features: a CPU torch tensor fp32 or fp16 [N,D]; seen bool [N]; the options of sparse.fuse.  misaligned: the
    device copy of features is a view one element into a larger buffer (base 4-byte aligned only)."""

    def __init__(self, name, batch, features, seen, n_split=None, num_files=1, seed=0, dtype=torch.float16, misaligned=False, **notes):
        self.name, self.n_split, self.num_files, self.seed, self.dtype, self.misaligned = name, n_split, num_files, seed, dtype, misaligned
        self.batch = np.ascontiguousarray(batch, np.int64)
        self.N = len(self.batch)
        rng = np.random.default_rng(len(name) + self.N)                # (x, y, z: fuse reads the batch column only)
        self.points = np.concatenate([self.batch[:, None].astype(np.float64), rng.uniform(0, 3, (self.N, 3))], 1)
        self.features = features
        self.seen = np.ascontiguousarray(seen, bool)
        self.D = features.shape[1]
        self.B = int(self.batch.max()) + 1
        self.notes = notes
        assert features.shape == (self.N, self.D) and self.seen.shape == (self.N,) and self.N <= 6000 and self.D <= 520

    def rows_of(self, b):
        return np.nonzero(self.batch == b)[0]


class Reference:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def reference_of(c, form):
    """mask_full bool [F,N], feat torch [R,D], offsets i64 [F,B+1], mask bool [R] or None, files {(b, k): the dict the reader loads}"""
    assert form in FORMS
    F, B = c.num_files, c.B
    mask_full = np.zeros((F, c.N), bool)
    offsets = np.zeros((F, B + 1), np.int64)
    rows_all, files, at = [], {}, 0
    for k in range(F):
        for b in range(B):
            rows = c.rows_of(b)
            ch = chunk(c.seed, b, k, len(rows), c.n_split)
            mf = ch & c.seen[rows] if form == "merged" else ch
            mask_full[k, rows] = mf
            offsets[k, b] = at
            at += int(mf.sum())
            rows_all.append(rows[mf])
            d = {"feat": c.features[torch.from_numpy(rows[mf])].to(c.dtype), "mask_full": torch.from_numpy(mf.copy())}
            if form == "chunk":
                d["mask"] = torch.from_numpy(c.seen[rows[mf]].copy())
            files[(b, k)] = d
        offsets[k, B] = at
    rows_all = np.concatenate(rows_all) if rows_all else np.zeros(0, np.int64)
    feat = c.features[torch.from_numpy(rows_all)].to(c.dtype)
    mask = c.seen[rows_all] if form == "chunk" else None
    return Reference(mask_full=mask_full, feat=feat, offsets=offsets, mask=mask, files=files, rows=rows_all)


_REFERENCES = {}


def reference(name, form):
    """computed once, shared, left unchanged"""
    if (name, form) not in _REFERENCES:
        _REFERENCES[(name, form)] = reference_of(case(name), form)
    return _REFERENCES[(name, form)]


# ------------------------------------------------------------------------------------------ the cases
# entry sizes around the wave (63 / 64 / 65), more than one block (257, 1025, 2500); entry 6 has no points (a gap), entry 8 nothing seen
SIZES = {0: 1, 1: 63, 2: 64, 3: 65, 4: 257, 5: 1025, 7: 2500, 8: 300}
LARGEST, UNSEEN_ENTRY, GAP_ENTRY = 7, 8, 6
SPLITS = {"1": 1, "64": 64, "nb1": SIZES[LARGEST] - 1, "none": None}
SEEDS = {"s0": 0, "s1": 1, "sbig": 2 ** 63 + 5}

# values at the conversion's edges: the largest half, just below the tie to inf, the tie itself, a tie to even, the smallest
# subnormal, the tie to zero below it, a subnormal, -0.0, the infinities and NaN
EDGE_VALUES = [65504.0, 65519.996, 65520.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 6e-8, 2.98e-8, 2.0 ** -25, 1e-6, -0.0, 0.0, float("inf"),
               float("-inf"), float("nan"), -65520.0, 1e30, -1e-30]


def _interleaved(sizes, rng):
    batch = np.concatenate([np.full(n, b, np.int64) for b, n in sizes.items()])
    return batch[rng.permutation(len(batch))]


def _features(n, d, rng, half=False):
    f = torch.from_numpy((rng.standard_normal((n, d)) * 3).astype(np.float32))
    return f.half() if half else f


def _selection(name):
    _, split, files, seed = name.split("_")
    rng = np.random.default_rng(11)
    batch = _interleaved(SIZES, rng)
    seen = rng.random(len(batch)) < 0.7
    seen[batch == UNSEEN_ENTRY] = False
    return Case(name, batch, _features(len(batch), 8, rng), seen, n_split=SPLITS[split], num_files=int(files[1:]), seed=SEEDS[seed])


WIDTH_SIZES = {0: 130, 1: 65, 2: 1}                               # n_split = 64: two entries select; the final file is one row


def _width(name, d, half_in=False, dtype=torch.float16, misaligned=False):
    rng = np.random.default_rng(100 + d)
    batch = _interleaved(WIDTH_SIZES, rng)
    seen = rng.random(len(batch)) < 0.8
    seen[batch == 2] = True
    return Case(name, batch, _features(len(batch), d, rng, half_in), seen, n_split=64, num_files=3, seed=7, dtype=dtype, misaligned=misaligned)


def _values(name):
    rng = np.random.default_rng(5)
    batch = _interleaved({0: 40, 1: 28}, rng)
    f = _features(len(batch), 4, rng)
    flat = f.reshape(-1)
    flat[:len(EDGE_VALUES)] = torch.tensor(EDGE_VALUES, dtype=torch.float32)
    flat[100:100 + len(EDGE_VALUES)] = -torch.tensor(EDGE_VALUES, dtype=torch.float32)
    return Case(name, batch, f, np.ones(len(batch), bool), dtype=torch.float16 if name == "values" else torch.float32)


def _loader(name):
    """two scenes with room-sized coordinates, for the project's FusedFeatureLoader on the saved files"""
    rng = np.random.default_rng(21)
    batch = _interleaved({0: 400, 1: 300}, rng)
    seen = rng.random(len(batch)) < 0.75
    c = Case(name, batch, _features(len(batch), 16, rng), seen, n_split=250, num_files=2 if name == "loader_2key" else 1, seed=3)
    c.colors = rng.uniform(-1, 1, (c.N, 3)).astype(np.float32)
    c.labels = rng.integers(0, 20, c.N).astype(np.int64)
    c.scene_names = ["scene0001_00", "scene0002_00"]
    return c


WIDTHS = (1, 3, 4, 6, 8, 12, 64, 260, 512, 520)
_BUILDERS = {}
for _split in SPLITS:
    for _files, _seed in (("f1", "s0"), ("f3", "s0"), ("f3", "s1"), ("f3", "sbig")):
        _BUILDERS[f"sel_{_split}_{_files}_{_seed}"] = _selection
for _d in WIDTHS:
    _BUILDERS[f"d{_d}"] = lambda name, d=_d: _width(name, d)
_BUILDERS["misaligned_d8"] = lambda name: _width(name, 8, misaligned=True)
_BUILDERS["misaligned_d520"] = lambda name: _width(name, 520, misaligned=True)
_BUILDERS["half_in_d8"] = lambda name: _width(name, 8, half_in=True)
_BUILDERS["half_in_d12"] = lambda name: _width(name, 12, half_in=True)
_BUILDERS["half_in_d3"] = lambda name: _width(name, 3, half_in=True)
_BUILDERS["f32_out_d8"] = lambda name: _width(name, 8, dtype=torch.float32)
_BUILDERS["f32_out_d6"] = lambda name: _width(name, 6, dtype=torch.float32)
_BUILDERS["half_in_f32_out_d8"] = lambda name: _width(name, 8, half_in=True, dtype=torch.float32)
_BUILDERS["half_in_f32_out_d3"] = lambda name: _width(name, 3, half_in=True, dtype=torch.float32)
_BUILDERS["values"] = _values
_BUILDERS["values_f32_out"] = _values
_BUILDERS["loader_2key"] = _loader
_BUILDERS["loader_3key"] = _loader

CASES = tuple(_BUILDERS)
SELECTION = tuple(n for n in CASES if n.startswith("sel_"))
LOADER = ("loader_2key", "loader_3key")
# the threshold key's top byte: the first and the last radix digit
TOP_BYTE_00 = tuple(n for n in SELECTION if n.split("_")[1] == "1")
TOP_BYTE_FF = tuple(n for n in SELECTION if n.split("_")[1] == "nb1")

_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name](name)
    return _CASES[name]
