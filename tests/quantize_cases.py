"""Cases and numpy oracle for the quantisation of batched point clouds (geopurify_amd.sparse.quantize, gp_quantize_batched,
gp_segment_labels).  Imported by test_quantize_cases_host.py (CPU) and test_gpu_quantize.py; no torch, no GPU.

Oracle:
  * unique rows, first index and inverse: np.unique(C, axis=0, return_index=True, return_inverse=True) -- rows in LEXICOGRAPHIC order,
    which is not the device's (ascending batch << 48 | morton key); `to_device_rows` renumbers the oracle by a device row order.
  * averages: accumulated in fp32, one point row at a time in ascending input row, then one fp32 division by the count -- the stated
    order of gp_scatter_mean_csr, so the device result is compared bit for bit.
  * labels: the three collision rules in plain numpy.
"""
import numpy as np

IGNORE = 255


# ------------------------------------------------------------------------------------------ cases
def _blob(rng, n, n_cells, lo=-40, ext=14, batches=(0, 1)):
    """n rows drawn (with repetition) from n_cells distinct cells of a blob with negative coordinates, over the given batch indices"""
    cells = np.unique(np.c_[rng.choice(batches, size=4 * n_cells), rng.integers(lo, lo + ext, size=(4 * n_cells, 3))], axis=0)
    cells = cells[rng.permutation(len(cells))[:n_cells]]
    rows = np.r_[np.arange(len(cells)), rng.integers(0, len(cells), size=max(n - len(cells), 0))][:n]
    return cells[rows[rng.permutation(n)]].astype(np.int32)


def _segments(rng, n_target):
    """about n_target rows in voxels of 1..5 rows each: in key order the segments straddle the 256-row block edges of the head-flag
    pass at arbitrary offsets"""
    sizes = rng.integers(1, 6, size=n_target // 3)
    cells = np.unique(np.c_[rng.integers(0, 3, size=4 * len(sizes)), rng.integers(-30, 30, size=(4 * len(sizes), 3))], axis=0)
    cells = cells[rng.permutation(len(cells))[:len(sizes)]]
    C = np.repeat(cells, sizes, axis=0)
    return C[rng.permutation(len(C))].astype(np.int32)


def _three_batches(rng):
    """batch indices 0, 5 and 65535; entries 0 and 65535 share every xyz (and entry 5 some of them): equal xyz must not merge across
    entries, duplicate rows inside an entry must"""
    a = np.unique(rng.integers(-6, 6, size=(120, 3)), axis=0)
    b = np.r_[a[:30], np.unique(rng.integers(20, 30, size=(60, 3)), axis=0)]
    C = np.concatenate([np.c_[np.full(len(e), i), e] for i, e in ((0, a), (5, b), (65535, a), (0, a[:40]), (65535, a[10:25]))])
    return C[rng.permutation(len(C))].astype(np.int32)


def _extent(rng, ext, axis):
    """an axis whose extent (max - min + 1) is exactly `ext`, with negative coordinates and some duplicate rows"""
    C = _blob(rng, 300, 120)
    C[0, 1 + axis] = -20000
    C[1, 1 + axis] = -20000 + ext - 1
    C[2] = C[1]
    return C


def cases():
    """name -> coordinates int32 [n, 4]; deterministic"""
    rng = np.random.default_rng(20240518)
    out = {}
    for n in (1, 255, 256, 257, 700):
        out[f"n{n}"] = _blob(rng, n, max(1, n // 3))
    d = np.unique(np.c_[rng.integers(0, 2, size=4000), rng.integers(-40, 40, size=(4000, 3))], axis=0)
    out["distinct700"] = d[rng.permutation(len(d))[:700]].astype(np.int32)            # nv = n
    out["identical700"] = np.tile(np.array([[3, -7, 11, -2]], np.int32), (700, 1))     # nv = 1: one 700-row segment
    out["segments2000"] = _segments(rng, 2000)
    out["batches_0_5_65535"] = _three_batches(rng)
    out["extent65535_y"] = _extent(rng, 65535, 1)                                      # the largest extent 16 bits per axis hold
    return out


def rejected_cases():
    """name -> (coordinates, axis letter): an extent of exactly 65536 is one too many"""
    rng = np.random.default_rng(7)
    return {"extent65536_z": (_extent(rng, 65536, 2), "z"), "extent65536_x": (_extent(rng, 65536, 0), "x")}


def features(name, n, d):
    """fp32 [n, d], deterministic per (case, d); magnitudes spread over a few binades so that the summation order shows"""
    rng = np.random.default_rng(len(name) * 1000003 + n * 1009 + d)
    return (rng.normal(0, 1, size=(n, d)) * np.exp2(rng.integers(-3, 4, size=(n, 1)))).astype(np.float32)


def labels(C, seed=0):
    """int64 [n]: mostly one label per voxel (so that "differ" keeps labels), every fifth point redrawn, some points already IGNORE"""
    rng = np.random.default_rng(1000 + seed + len(C))
    o = Oracle(C)
    lab = rng.integers(0, 20, size=o.nv)[o.inverse]
    redraw = rng.random(len(C)) < 0.2
    lab[redraw] = rng.integers(0, 20, size=int(redraw.sum()))
    lab[rng.random(len(C)) < 0.05] = IGNORE
    return lab.astype(np.int64)


# ------------------------------------------------------------------------------------------ oracle
class Oracle:
    """np.unique of the rows: coordinates [nv, 4] (lexicographic), unique_index [nv] (first = lowest input row), inverse [n], counts"""

    def __init__(self, C):
        C = np.asarray(C)
        self.C = C
        self.coordinates, self.unique_index, inverse = np.unique(C, axis=0, return_index=True, return_inverse=True)
        self.inverse = inverse.reshape(-1)
        self.n, self.nv = len(C), len(self.coordinates)
        self.counts = np.bincount(self.inverse, minlength=self.nv)

    def to_device_rows(self, device_coordinates):
        """The oracle renumbered by a device row order: device_coordinates [nv, 4] must hold exactly the oracle's rows (asserted).
        -> Oracle-like object whose voxel v is device row v."""
        dc = np.asarray(device_coordinates)
        assert dc.shape == self.coordinates.shape, (dc.shape, self.coordinates.shape)
        lex = np.lexsort(dc.T[::-1])                                # device rows in lexicographic order
        assert np.array_equal(dc[lex], self.coordinates), "the device's rows are not the unique rows"
        o = object.__new__(Oracle)
        o.C, o.n, o.nv = self.C, self.n, self.nv
        o.coordinates = dc
        o.unique_index = np.empty_like(self.unique_index)
        o.unique_index[lex] = self.unique_index
        o.counts = np.empty_like(self.counts)
        o.counts[lex] = self.counts
        o.inverse = lex[self.inverse]
        return o

    def average(self, F):
        """fp32 [nv, d]: fp32 sums in ascending input row, one fp32 division"""
        F = np.asarray(F, dtype=np.float32)
        acc = np.zeros((self.nv, F.shape[1]), dtype=np.float32)
        for i in range(self.n):
            acc[self.inverse[i]] += F[i]
        return acc / self.counts.astype(np.float32)[:, None]

    def mean_f64(self, F):
        acc = np.zeros((self.nv, F.shape[1]), dtype=np.float64)
        np.add.at(acc, self.inverse, np.asarray(F, dtype=np.float64))
        return acc / self.counts[:, None]

    def mean_abs_f64(self, F):
        return self.mean_f64(np.abs(np.asarray(F, dtype=np.float64)))

    def subsample(self, F):
        return np.asarray(F)[self.unique_index]

    def labels(self, lab, rule, ignore=IGNORE):
        lab = np.asarray(lab, dtype=np.int64)
        first = lab[self.unique_index]
        if rule == "first":
            return first
        if rule == "count":
            return np.where(self.counts > 1, ignore, first)
        if rule == "differ":
            differs = np.zeros(self.nv, dtype=bool)
            np.logical_or.at(differs, self.inverse, lab != first[self.inverse])
            return np.where(differs, ignore, first)
        raise ValueError(rule)
