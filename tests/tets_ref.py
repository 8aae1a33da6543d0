"""Reference for radfoam.delaunay_tets (helper, no GPU): Qhull's simplices canonicalised with exact signs (Fractions of
the float32 inputs), vert_to_tet and tet_adjacency by dictionaries over the faces, the hull facet count from
scipy.spatial.Delaunay(...).convex_hull; the clouds the CPU and GPU tests share; the checks both run."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

NONE = 0xFFFFFFFF


# ---- the clouds -------------------------------------------------------------------------------------------------------

def uniform(n, seed=0):
    return np.random.default_rng(seed).uniform(-1, 1, (n, 3)).astype(np.float32)


def clustered(n, seed=1):
    """clusters over three decades of scale, the kind of tests/test_delaunay.py"""
    rng = np.random.default_rng(seed)
    per = -(-n // 5)
    pts = np.concatenate([rng.normal(0, s, size=(per, 3)) + rng.uniform(-1, 1, 3) for s in (1.0, 0.1, 0.01, 0.001, 0.3)])
    return pts[:n].astype(np.float32)


def sheet(n, seed=2):
    """every point on the rim: a sphere shell a thousandth thick"""
    rng = np.random.default_rng(seed)
    shell = rng.normal(size=(n, 3))
    shell /= np.linalg.norm(shell, axis=1, keepdims=True)
    return (shell * (1 + 1e-3 * rng.normal(size=(n, 1)))).astype(np.float32)


def offset(n, seed=3):
    return (uniform(n, seed).astype(np.float64) + 1000.0).astype(np.float32)


def scaled(n, seed=4):
    return (uniform(n, seed).astype(np.float64) * 1e-3).astype(np.float32)


def hub(k, seed=5):
    """a site (index 0) at the centre of k points on a sphere, plus 100 points outside"""
    rng = np.random.default_rng(seed)
    shell = rng.normal(size=(k, 3))
    shell /= np.linalg.norm(shell, axis=1, keepdims=True)
    outside = rng.normal(size=(100, 3))
    outside *= rng.uniform(1.6, 3.0, size=(100, 1)) / np.linalg.norm(outside, axis=1, keepdims=True)
    return np.concatenate([np.zeros((1, 3)), shell * (1 + 1e-4 * rng.normal(size=(k, 1))), outside]).astype(np.float32)


def lattice(k=4):
    return np.stack(np.meshgrid(*[np.arange(k)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


KINDS = {"uniform": uniform, "clustered": clustered, "sheet": sheet, "offset": offset, "scaled": scaled}
SIZES = (33, 64, 65, 400, 3000)
CLOUDS = [(kind, n) for kind in KINDS for n in SIZES]
_REF = {}


# ---- the reference ----------------------------------------------------------------------------------------------------

def _sign(points, row):
    f = [[Fraction(float(x)) for x in points[s]] for s in row]
    a, b, c = ([f[k][d] - f[0][d] for d in range(3)] for k in (1, 2, 3))
    det = a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0])
    return (det > 0) - (det < 0)


def exact_signs(points, rows):
    """the exact sign of det[p1 - p0; p2 - p0; p3 - p0] of every row"""
    return np.array([_sign(points, [int(s) for s in row]) for row in rows], dtype=np.int64)


def lists_of(simplices, n):
    """(adjacency uint32[E], offsets uint32[N+1]) of a set of tetrahedra, every row ascending"""
    s = np.asarray(simplices, dtype=np.int64)
    pairs = s[:, [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]].reshape(-1, 2)
    code = np.unique(np.concatenate([pairs[:, 0] * n + pairs[:, 1], pairs[:, 1] * n + pairs[:, 0]]))
    offsets = np.searchsorted(code // n, np.arange(n + 1))
    return (code % n).astype(np.uint32), offsets.astype(np.uint32)


def reference(points) -> dict:
    """dict(points, adjacency, offsets, tets int64[T,4], vert_to_tet int64[N], tet_adjacency int64[T,4] (-1 on the hull),
    hull_faces, simplices) of float32 points through Qhull"""
    from scipy.spatial import Delaunay

    pts = np.ascontiguousarray(points, dtype=np.float32)
    n = len(pts)
    mesh = Delaunay(pts.astype(np.float64))
    rows = [sorted(int(s) for s in simplex) for simplex in mesh.simplices]
    rows.sort()
    out = []
    for row in rows:
        sign = _sign(pts, row)
        assert sign != 0, "Qhull returned a flat tetrahedron"
        out.append(row if sign > 0 else [row[0], row[1], row[3], row[2]])
    tets = np.array(out, dtype=np.int64).reshape(-1, 4)
    vert_to_tet = np.full(n, -1, dtype=np.int64)
    faces = {}
    for t, row in enumerate(out):
        for j, s in enumerate(row):
            if vert_to_tet[s] < 0:
                vert_to_tet[s] = t
            faces.setdefault(tuple(sorted(row[:j] + row[j + 1:])), []).append(4 * t + j)
    tet_adjacency = np.full(4 * len(out), -1, dtype=np.int64)
    for pair in faces.values():
        assert len(pair) <= 2
        if len(pair) == 2:
            tet_adjacency[pair[0]], tet_adjacency[pair[1]] = pair[1], pair[0]
    adjacency, offsets = lists_of(mesh.simplices, n)
    return dict(points=pts, adjacency=adjacency, offsets=offsets, tets=tets, vert_to_tet=vert_to_tet,
                tet_adjacency=tet_adjacency.reshape(-1, 4), hull_faces=len(mesh.convex_hull), simplices=mesh.simplices)


def cloud(kind, n) -> dict:
    """the reference of a named cloud, computed once and shared; callers leave it unchanged"""
    if (kind, n) not in _REF:
        pts = hub(n) if kind == "hub" else lattice(n) if kind == "lattice" else KINDS[kind](n)
        _REF[(kind, n)] = reference(pts)
    return _REF[(kind, n)]


# ---- the checks -------------------------------------------------------------------------------------------------------

def _signed(x):
    """uint32 tables with 0xFFFFFFFF as int64 with -1"""
    x = np.asarray(x).astype(np.int64)
    return np.where(x == NONE, -1, x)


def check_against(ref: dict, tets, vert_to_tet, tet_adjacency, hull_faces):
    """Everything the issue asks of a result: rows equal to the reference's row for row and corner for corner, strictly
    ascending, every sign exactly positive, vert_to_tet and tet_adjacency equal, tet_adjacency an involution over equal
    faces, hull_faces Qhull's."""
    tets = np.asarray(tets).astype(np.int64)
    assert tets.shape == ref["tets"].shape and np.array_equal(tets, ref["tets"])
    check_rows(ref["points"], tets)
    assert np.array_equal(_signed(vert_to_tet), ref["vert_to_tet"])
    assert hull_faces == ref["hull_faces"]
    if tet_adjacency is not None:
        adj = _signed(tet_adjacency)
        assert np.array_equal(adj, ref["tet_adjacency"])
        check_involution(tets, adj)


def check_rows(points, tets):
    tets = np.asarray(tets).astype(np.int64)
    keys = np.sort(tets, axis=1)
    assert (keys[:, 0] == tets[:, 0]).all() and (keys[:, 1] == tets[:, 1]).all()
    later = keys[1:], keys[:-1]
    differ = later[0] != later[1]
    first = differ.argmax(1)
    rows = np.arange(len(keys) - 1)
    assert differ.any(1).all() and (later[0][rows, first] > later[1][rows, first]).all(), "rows not strictly ascending"
    assert (exact_signs(points, tets) == 1).all()


def check_involution(tets, adj):
    flat = adj.reshape(-1)
    inner = np.nonzero(flat >= 0)[0]
    assert np.array_equal(flat[flat[inner]], inner)
    faces = np.sort(tets[:, [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]]], axis=2).reshape(-1, 3)
    assert np.array_equal(faces[inner], faces[flat[inner]])


# ---- malformed and stale lists, the lattice -----------------------------------------------------------------------------

def _row(ref, i):
    return ref["adjacency"][int(ref["offsets"][i]):int(ref["offsets"][i + 1])].astype(np.int64)


def _with_row(ref, i, row):
    """the lists with row i replaced"""
    adj, off = ref["adjacency"].astype(np.int64), ref["offsets"].astype(np.int64)
    a, b = off[i], off[i + 1]
    off = off.copy()
    off[i + 1:] += len(row) - (b - a)
    return np.concatenate([adj[:a], np.asarray(row, dtype=np.int64), adj[b:]]), off


def malformed_lists(ref, i=7):
    """name -> (adjacency, offsets), each a RuntimeError"""
    n, row = len(ref["points"]), _row(ref, i)
    swapped = ref["offsets"].astype(np.int64).copy()
    swapped[[i, i + 1]] = swapped[[i + 1, i]]
    return {"self": _with_row(ref, i, np.r_[row, i]), "twice": _with_row(ref, i, np.r_[row, row[0]]),
            "above": _with_row(ref, i, np.r_[row[:-1], n]), "below": _with_row(ref, i, np.r_[row[:-1], -1]),
            "offsets": (ref["adjacency"].astype(np.int64), swapped),
            "short": (ref["adjacency"].astype(np.int64)[:-1], ref["offsets"].astype(np.int64))}


def stale_lists(ref, i=7):
    """name -> (adjacency, offsets), each a TriangulationFailedError: one true neighbour removed from a row, one
    non-neighbour added to it"""
    n, row = len(ref["points"]), _row(ref, i)
    stranger = next(j for j in range(n) if j != i and j not in set(row.tolist()))
    return {"removed": _with_row(ref, i, row[1:]), "added": _with_row(ref, i, np.r_[row, stranger])}


def lattice_outcome(run):
    """The 4x4x4 lattice with Qhull's lists: cospherical points are never in strict conflict, so the stars may disagree
    with Qhull's choice of diagonals.  Either the call raises TriangulationFailedError or what it returns passes every
    check.  Returns which."""
    from scipy.spatial import Delaunay

    from radfoam_amd.triangulation import TriangulationFailedError
    pts = lattice(4)
    simplices = Delaunay(pts.astype(np.float64)).simplices
    adj, off = lists_of(simplices, len(pts))
    try:
        tets, vert_to_tet, tet_adjacency, hull_faces = run(pts, adj, off)
    except TriangulationFailedError:
        return "raised"
    tets = np.asarray(tets).astype(np.int64)
    check_rows(pts, tets)
    adj_out = _signed(tet_adjacency)
    check_involution(tets, adj_out)
    assert hull_faces == int((adj_out < 0).sum())
    first = np.full(len(pts), -1, dtype=np.int64)
    for t in range(len(tets) - 1, -1, -1):
        first[tets[t]] = t
    assert np.array_equal(_signed(vert_to_tet), first)
    got_adj, got_off = lists_of(tets, len(pts))
    assert np.array_equal(got_adj, adj) and np.array_equal(got_off, off)
    return "returned"
