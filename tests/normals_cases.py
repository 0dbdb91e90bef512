"""Cases and numpy references for the geometry channels: sparse.mesh_normals, ops.knn_normals, sparse.estimate_normals
(csrc/normals.hip).  CPU only; tests/test_normals_cases_host.py checks the references against each other and against the golden of
the reference's own function, tests/test_gpu_normals.py compares the kernels with them.

Mesh.  vertex_normal_loop restates models/utils/mapping_util.py:9-29 with every operation written out in the order numpy takes it
(np.cross: each product rounded, then the difference; np.sum over three elements: (x0 + x1) + x2; the buffered nv[face[i]] += nf[i]
as read-add-write, once per distinct vertex), so it does not depend on how a numpy version reduces; mesh_reference runs it per entry
with local indices.  All comparisons with it are on bit patterns.

Neighbour-list normals.  knn_normals_reference takes the fp64 sums in the kernel's order, then np.linalg.eigh; its gap and sign_free
name the rows whose eigenvector or sign is ill-conditioned (compared up to sign or not at all, at most 1 % of the corner cases).
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DTYPES = (np.float32, np.float64)
INT_OF = {np.dtype(np.float32): np.int32, np.dtype(np.float64): np.int64}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(INT_OF[a.dtype])


# ------------------------------------------------------------------------------------------ the restated reference
def face_contributions(vertex, face):
    """nf * area of mapping_util.py:9-21, [F,3] in vertex's dtype"""
    T = vertex.dtype.type
    p0, p1, p2 = vertex[face[:, 0]], vertex[face[:, 1]], vertex[face[:, 2]]
    a, b = p1 - p0, p2 - p0
    vec = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    sq = vec * vec
    length = np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2]) + T(1.0e-8)
    nf = vec / length[:, None]
    area = length * T(0.5)
    out = nf * area[:, None]
    assert out.dtype == vertex.dtype
    return out


def vertex_normal_loop(vertex, face):
    """mapping_util.vertex_normal (:19-29) on one mesh, in vertex's dtype"""
    T = vertex.dtype.type
    c = face_contributions(vertex, face)
    nv = np.zeros_like(vertex)
    for i in range(face.shape[0]):
        for v in dict.fromkeys(face[i].tolist()):                  # a vertex named twice is written once
            nv[v] = nv[v] + c[i]
    sq = nv * nv
    length = np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2]) + T(1.0e-8)
    return nv / length[:, None]


def mesh_reference(points, faces):
    """points [N,4] (batch, x, y, z) of one dtype, faces [F,3] of rows of points -> [N,3]: per entry vertex_normal_loop on that entry
    alone with local indices (its faces in their order among all faces); rows that no entry's mesh holds stay zero"""
    out = np.zeros((len(points), 3), points.dtype)
    face_entry = points[faces[:, 0], 0]
    assert np.array_equal(points[faces[:, 1], 0], face_entry) and np.array_equal(points[faces[:, 2], 0], face_entry)
    for b in np.unique(points[:, 0]):
        rows = np.flatnonzero(points[:, 0] == b)
        local = np.full(len(points), -1, np.int64)
        local[rows] = np.arange(len(rows))
        f = local[faces[face_entry == b]]
        if len(f):
            out[rows] = vertex_normal_loop(np.ascontiguousarray(points[rows, 1:]), f)
    return out


# ------------------------------------------------------------------------------------------ mesh cases
def grid_mesh(rng, nu, nv, pitch=0.05, jitter=0.3, relief=0.02):
    """a jittered height field of nu x nv vertices, two triangles per cell, the faces in random order -> (xyz f64 [nu*nv,3], faces)"""
    gu, gv = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    xyz = np.stack([gu.reshape(-1) * pitch, gv.reshape(-1) * pitch, np.zeros(nu * nv)], 1)
    xyz[:, :2] += rng.uniform(-jitter, jitter, (nu * nv, 2)) * pitch
    xyz[:, 2] = rng.normal(0, relief, nu * nv)
    idx = np.arange(nu * nv).reshape(nu, nv)
    a, b, c, d = idx[:-1, :-1].reshape(-1), idx[1:, :-1].reshape(-1), idx[1:, 1:].reshape(-1), idx[:-1, 1:].reshape(-1)
    faces = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])
    return xyz, faces[rng.permutation(len(faces))].astype(np.int64)


def fan_mesh(rng, valence):
    """a hub (vertex 0) in `valence` faces over a closed ring, the ring lifted off the plane -> (xyz, faces)"""
    ang = np.linspace(0, 2 * np.pi, valence, endpoint=False)
    ring = np.stack([np.cos(ang), np.sin(ang), rng.normal(0, 0.2, valence)], 1) * rng.uniform(0.5, 1.5, (valence, 1))
    xyz = np.concatenate([[[0.0, 0.0, 0.3]], ring])
    r = 1 + np.arange(valence)
    faces = np.stack([np.zeros(valence, np.int64), r, 1 + (np.arange(valence) + 1) % valence], 1)
    return xyz, faces[rng.permutation(valence)].astype(np.int64)


def odd_mesh(rng):
    """a small grid plus: two vertices of no face, a lone triangle (three vertices of valence 1), a zero-area face (two corners at one
    position), a face with collinear corners, a face that names a vertex twice, a face listed twice"""
    xyz, faces = grid_mesh(rng, 6, 5)
    n = len(xyz)
    extra = np.array([[9.0, 9.0, 9.0], [8.0, 9.0, 7.0],                                   # n, n + 1: valence 0
                      [5.0, 5.0, 0.0], [5.5, 5.0, 0.1], [5.0, 5.5, 0.2],                  # n + 2 .. n + 4: the lone triangle
                      xyz[3],                                                            # n + 5: the position of vertex 3
                      [1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [3.0, 3.0, 3.0]])                # n + 6 .. n + 8: collinear
    more = np.array([[n + 2, n + 3, n + 4], [3, n + 5, 7], [n + 6, n + 7, n + 8], [4, 4, 9], [11, 12, 11], faces[2], faces[2]], np.int64)
    faces = np.concatenate([faces, more])
    return np.concatenate([xyz, extra]), faces[rng.permutation(len(faces))]


class Mesh:
    def __init__(self, points, faces):
        self.points, self.faces = points, faces                    # points f64 [N,4]; a test casts them to its dtype

    def cast(self, dtype):
        return np.ascontiguousarray(self.points.astype(dtype))


def _single(xyz, faces, batch=0):
    return Mesh(np.column_stack([np.full(len(xyz), float(batch)), xyz]), faces)


def interleave(meshes, rng):
    """the meshes as entries 0, 1, .. of one cloud: their rows interleaved by a random permutation, their faces interleaved by a
    random merge that keeps every mesh's own face order -> (Mesh, rows: per mesh the rows of its vertices)"""
    sizes = [len(m.points) for m in meshes]
    owner = rng.permutation(np.repeat(np.arange(len(meshes)), sizes))
    rows = [np.flatnonzero(owner == b) for b in range(len(meshes))]
    points = np.zeros((len(owner), 4))
    for b, m in enumerate(meshes):
        points[rows[b], 0] = b
        points[rows[b], 1:] = m.points[:, 1:]
    fowner = rng.permutation(np.repeat(np.arange(len(meshes)), [len(m.faces) for m in meshes]))
    faces = np.zeros((len(fowner), 3), np.int64)
    for b, m in enumerate(meshes):
        faces[fowner == b] = rows[b][m.faces]
    return Mesh(points, faces), rows


@functools.lru_cache(maxsize=None)
def mesh_case(name):
    rng = np.random.default_rng({"grid": 11, "fan65": 12, "fan300": 13, "odd": 14, "three": 15}[name])
    if name == "grid":
        return _single(*grid_mesh(rng, 18, 17))                    # 306 vertices, 544 faces: more than one block of each kernel
    if name == "fan65":
        return _single(*fan_mesh(rng, 70))                         # the hub's list is longer than a wave
    if name == "fan300":
        return _single(*fan_mesh(rng, 300))                        # ... and than a block
    if name == "odd":
        return _single(*odd_mesh(rng))
    if name == "three":
        return interleave([mesh_case("odd"), mesh_case("fan65"), _single(*grid_mesh(rng, 7, 9))], rng)[0]
    raise KeyError(name)


MESH_CASES = ("grid", "fan65", "fan300", "odd", "three")


def three_parts():
    """the three meshes of case "three" on their own and the rows they take in it"""
    rng = np.random.default_rng(15)
    parts = [mesh_case("odd"), mesh_case("fan65"), _single(*grid_mesh(rng, 7, 9))]
    whole, rows = interleave(parts, rng)
    assert np.array_equal(whole.points, mesh_case("three").points) and np.array_equal(whole.faces, mesh_case("three").faces)
    return parts, rows


def valence(faces, n):
    """per vertex the number of faces that name it (a face that names it twice counted once)"""
    val = np.zeros(n, np.int64)
    for f in faces:
        for v in set(f.tolist()):
            val[v] += 1
    return val


def order_preserving_permutation(faces, rng):
    """a permutation of the face rows under which every vertex sees its faces in the same order: neighbouring rows that share no
    vertex swapped, at random -> perm (faces[perm] is the permuted list), with at least one swap"""
    perm = np.arange(len(faces))
    i, swaps = 0, 0
    while i + 1 < len(faces):
        if not set(faces[i].tolist()) & set(faces[i + 1].tolist()) and rng.random() < 0.8:
            perm[i], perm[i + 1] = i + 1, i
            swaps += 1
            i += 2
        else:
            i += 1
    assert swaps > 0
    return perm


def vertex_orders(faces, n):
    """per vertex the tuple of the CONTRIBUTIONS' identities in list order: (sorted corner tuple) per face, so that two listings of
    one face are the same item"""
    lists = [[] for _ in range(n)]
    for f in faces:
        for v in dict.fromkeys(f.tolist()):
            lists[v].append(tuple(f.tolist()))
    return lists


# ------------------------------------------------------------------------------------------ neighbour-list normals: the reference
EIG_GAP = 1e-3                                                      # (l1 - l0) / l2 below which the eigenvector is not compared
SIGN_MARGIN = 1e-6
EIG_TOL = 2.0 ** -23
UNIT_TOL = 2.0 ** -22


class KnnNormals:
    """what knn_normals_reference returns: normals f32 [n,3] and variation f32 [n] (rows with a bad index: zeros), evals f64 [n,3]
    ascending, gap f64 [n] = (l1 - l0) / l2 (0 where l2 == 0), sign_free bool [n] (the sign rule is within its margin), bad bool [n]"""

    def __init__(self, normals, variation, evals, gap, sign_free, bad):
        self.normals, self.variation, self.evals, self.gap, self.sign_free, self.bad = normals, variation, evals, gap, sign_free, bad


def knn_normals_reference(positions, neighbors, toward=None, toward_rows=None):
    """the definition, in fp64: the set is i then its listed rows, m = (sum p) / (k + 1), C = sum (p - m)(p - m)^T in that order,
    np.linalg.eigh; the sign rule applied to the fp32-rounded vector (largest magnitude) or in fp64 (toward)"""
    P = np.asarray(positions)[:, :3].astype(np.float64)
    nbr = np.asarray(neighbors).astype(np.int64)
    n, k = nbr.shape
    bad = ((nbr < 0) | (nbr >= n)).any(1)
    sets = np.concatenate([np.arange(n)[:, None], np.where((nbr < 0) | (nbr >= n), 0, nbr)], 1)
    Q = P[sets]                                                     # [n, k+1, 3]
    s = Q[:, 0].copy()
    for j in range(1, k + 1):
        s = s + Q[:, j]
    m = s / float(k + 1)
    D = Q - m[:, None]
    C = np.zeros((n, 3, 3))
    for j in range(k + 1):
        C = C + D[:, j, :, None] * D[:, j, None, :]
    w, V = np.linalg.eigh(C)
    vec = V[:, :, 0]
    vec = vec / np.linalg.norm(vec, axis=1, keepdims=True)
    l0 = np.maximum(w[:, 0], 0.0)
    total = (l0 + w[:, 1]) + w[:, 2]
    variation = np.where(total > 0, l0 / np.where(total > 0, total, 1.0), 0.0).astype(np.float32)
    gap = np.where(w[:, 2] > 0, (w[:, 1] - w[:, 0]) / np.where(w[:, 2] > 0, w[:, 2], 1.0), 0.0)
    out = vec.astype(np.float32)
    if toward is not None:
        t = np.asarray(toward, np.float64)[np.asarray(toward_rows)] - P
        dot = (vec * t).sum(1)
        flip = dot < 0
        sign_free = np.abs(dot) < SIGN_MARGIN * np.linalg.norm(t, axis=1)
    else:
        mag = np.abs(out)
        lead = mag.argmax(1)                                        # (the first among equals: the lowest axis)
        flip = out[np.arange(n), lead] < 0
        top2 = np.sort(mag, 1)
        sign_free = top2[:, 2] - top2[:, 1] < SIGN_MARGIN
    out = np.where(flip[:, None], -out, out)
    out[bad], variation[bad] = 0, 0
    return KnnNormals(out, variation, w, gap, sign_free, bad)


def compare_knn_normals(got_n, got_v, ref, what=""):
    """the bounds of the GPU test, on numpy arrays -> (rows compared exactly, rows compared up to sign, rows not compared)"""
    got_n, got_v = np.asarray(got_n), np.asarray(got_v)
    assert got_n.dtype == np.float32 and got_v.dtype == np.float32 and got_n.shape == ref.normals.shape and got_v.shape == ref.variation.shape, what
    assert np.isfinite(got_n).all() and np.isfinite(got_v).all(), what
    ok = ~ref.bad
    norm = np.linalg.norm(got_n[ok].astype(np.float64), axis=1)
    assert np.abs(norm - 1).max(initial=0) <= UNIT_TOL, (what, np.abs(norm - 1).max())
    assert not got_n[ref.bad].any() and not got_v[ref.bad].any(), what
    has = ok & (ref.evals[:, 2] > 0)
    dv = np.abs(got_v[has].astype(np.float64) - ref.variation[has]).max(initial=0)
    assert dv <= EIG_TOL, (what, "variation", dv)
    sure = ok & (ref.gap >= EIG_GAP)
    exact, loose = sure & ~ref.sign_free, sure & ref.sign_free
    d = np.abs(got_n[exact].astype(np.float64) - ref.normals[exact]).max(initial=0)
    assert d <= EIG_TOL, (what, "normals", d, int(np.abs(got_n[exact].astype(np.float64) - ref.normals[exact]).max(1).argmax()))
    if loose.any():
        a, b = got_n[loose].astype(np.float64), ref.normals[loose].astype(np.float64)
        d = np.minimum(np.abs(a - b).max(1), np.abs(a + b).max(1)).max()
        assert d <= EIG_TOL, (what, "normals up to sign", d)
    return int(exact.sum()), int(loose.sum()), int((ok & ~sure).sum())


# ------------------------------------------------------------------------------------------ neighbour-list cases
def brute_lists(xyz, k):
    """the k nearest other rows by (d^2, row), fp64 -> i64 [n,k]"""
    P = np.asarray(xyz, np.float64)
    d2 = ((P[:, None] - P[None]) ** 2).sum(2)
    np.fill_diagonal(d2, np.inf)
    return np.argsort(d2, axis=1, kind="stable")[:, :k].astype(np.int64)


def corner_points(rng, side, pitch=0.02):
    """three jittered planes of side x side samples meeting at right angles (jitter 0.4 pitch in the plane, 1.5 mm noise off it)
    -> f64 [3 * side^2, 3]"""
    g = (np.arange(side) + 0.5) * pitch
    u, v = (a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij"))
    planes = []
    for axis in range(3):
        p = np.zeros((side * side, 3))
        p[:, (axis + 1) % 3] = u + rng.uniform(-0.4, 0.4, side * side) * pitch
        p[:, (axis + 2) % 3] = v + rng.uniform(-0.4, 0.4, side * side) * pitch
        p[:, axis] = rng.normal(0, 0.0015, side * side)
        planes.append(p)
    return np.concatenate(planes)


def corner_cloud(rng, side, pitch=0.02, voxel=0.05):
    """corner_points reduced to the centroids of their `voxel` cells: voxel-like positions f64 [n,3]"""
    pts = corner_points(rng, side, pitch)
    cells = np.floor(pts / voxel).astype(np.int64)
    _, inverse, counts = np.unique(cells, axis=0, return_inverse=True, return_counts=True)
    cent = np.zeros((len(counts), 3))
    np.add.at(cent, inverse.reshape(-1), pts)
    return cent / counts[:, None]


CORNER_CASES = {"corner24_k3": (24, 3, 21), "corner24_k16": (24, 16, 22), "corner40_k16": (40, 16, 23), "corner40_k127": (40, 127, 24)}


class KnnCase:
    def __init__(self, positions, neighbors):
        self.positions, self.neighbors = positions, neighbors


@functools.lru_cache(maxsize=None)
def knn_case(name):
    """positions f64 [n,3] (a test rounds them to its dtype FIRST and hands the rounded values to the reference), lists i64 [n,k]"""
    if name in CORNER_CASES:
        side, k, seed = CORNER_CASES[name]
        P = corner_cloud(np.random.default_rng(seed), side)
        return KnnCase(P, brute_lists(P, k))
    if name == "line":                                              # collinear sets: l0 = l1 = 0, the direction is unspecified
        P = np.outer(np.arange(70.0), [0.03, 0.04, 0.12]) + [1.0, 2.0, 3.0]
        return KnnCase(P, brute_lists(P, 4))
    if name == "lattice":                                           # an exact flat patch: l0 = 0 exactly, and l1 = l2 in its interior
        g = np.arange(9.0) * 0.0625
        u, v = (a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij"))
        P = np.stack([u, v, np.full(81, 0.5)], 1)
        return KnnCase(P, brute_lists(P, 8))
    if name == "point":                                             # every listed row at the row's own position: C = 0
        P = np.tile([[0.25, -1.5, 3.0]], (67, 1))
        return KnnCase(P, brute_lists(P, 3))
    if name == "bad_index":
        c = knn_case("corner24_k16")
        nbr = c.neighbors.copy()
        nbr[37, 5] = len(c.positions)                               # one past the end, in one list
        return KnnCase(c.positions, nbr)
    raise KeyError(name)


def viewpoints(case, rng, per_row):
    """toward / toward_rows for a case: two viewpoints off the corner chosen per row at random, or one target per row"""
    n = len(case.positions)
    if per_row:
        return case.positions + rng.normal(0, 1.0, (n, 3)), np.arange(n)
    return np.array([[0.6, 0.5, 0.7], [1.5, 0.2, 0.4]]), rng.integers(0, 2, n)


# ------------------------------------------------------------------------------------------ estimate_normals: the chain in numpy
def estimate_reference(points, quantization_size, k):
    """quantize (floor division, voxels in ascending key order, fp32 sums in ascending point row and one division), the lattice kNN
    of the oracle inside each entry, knn_normals_reference (no toward) -> (KnnNormals, centroids f32 [nv,3], lists, inverse [N],
    coordinates i64 [nv,4])"""
    import knn_batched_cases as kb
    points = np.asarray(points)
    cells = np.floor_divide(points[:, 1:], points.dtype.type(quantization_size)).astype(np.int64)
    C = np.column_stack([points[:, 0].astype(np.int64), cells])
    keys = kb.keys_of(C)
    ukeys, inverse, counts = np.unique(keys, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    first = np.full(len(ukeys), len(points), np.int64)
    np.minimum.at(first, inverse, np.arange(len(points)))
    coords = C[first]
    acc = np.zeros((len(ukeys), 3), np.float32)
    np.add.at(acc, inverse, points[:, 1:].astype(np.float32))       # unbuffered: in ascending point row
    cent = acc / counts.astype(np.float32)[:, None]
    lists = kb.oracle_lists_of(coords, k)
    return knn_normals_reference(cent, lists), cent, lists, inverse, coords


def scene_interior(points_xyz, analytic, lists, inverse, plane_tol=0.008):
    """voxels away from patch borders: every point of the voxel and of its k listed voxels has one analytic normal n, and all of
    them lie within plane_tol of their common plane along n -> (bool [nv], analytic normal per voxel f64 [nv,3])"""
    nv = lists.shape[0]
    first = np.full(nv, len(inverse), np.int64)
    np.minimum.at(first, inverse, np.arange(len(inverse)))
    nrm = analytic[first]                                           # the voxel's candidate normal: its lowest point's
    same = np.ones(nv, bool)
    np.logical_and.at(same, inverse, (analytic == nrm[inverse]).all(1))
    off = (points_xyz * nrm[inverse]).sum(1)                        # offset along the voxel's normal
    lo, hi = np.full(nv, np.inf), np.full(nv, -np.inf)
    np.minimum.at(lo, inverse, off)
    np.maximum.at(hi, inverse, off)
    sets = np.concatenate([np.arange(nv)[:, None], lists], 1)
    ok = same[sets].all(1) & (nrm[sets] == nrm[:, None]).all(2).all(1)
    ok &= (hi[sets].max(1) - lo[sets].min(1)) <= 2 * plane_tol
    return ok, nrm


def angle_up_to_sign(a, b):
    c = np.abs((np.asarray(a, np.float64) * np.asarray(b, np.float64)).sum(1)) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    return np.arccos(np.clip(c, 0.0, 1.0))


SCENE_VOXEL, SCENE_K, SCENE_SEED = 0.07, 16, 123
# the worst angle (rad) between knn_normals_reference's voxel normals and the analytic normals of synthetic.make_scene(CONFIGS["T"], 123)
# over the interior voxels, measured by test_normals_cases_host.test_scene_angle_is_the_recorded_one (which recomputes it)
SCENE_WORST_ANGLE = 0.0180402                                      # over 716 interior voxels of 1813 (1.03 degrees)
