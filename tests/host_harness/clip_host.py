"""ctypes loader of the HOST build of radfoam_amd/csrc/rf_clip.hpp (test harness; see clip_host.cpp), and the Qhull
reference the cell-geometry tests compare against (scipy.spatial.Voronoi + ConvexHull per region, in double); the clouds
that stand on the kernel's seams, which are compared with the exact reference of tests/cell_geometry_ref.py instead."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libclip_host.so")
_SRC = [os.path.join(_HERE, "clip_host.cpp"), os.path.join(_HERE, "..", "..", "radfoam_amd", "csrc", "rf_clip.hpp")]


def build():
    if os.path.exists(_SO) and all(os.path.getmtime(s) <= os.path.getmtime(_SO) for s in _SRC):
        return _SO
    os.makedirs(os.path.dirname(_SO), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", _SO, _SRC[0]],
                   check=True)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.clip_host_cell_geometry.restype = C.c_int
        _lib.clip_host_cell_geometry.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                                 C.c_uint32] + [C.c_void_p] * 6
        _lib.clip_host_face_polygon.restype = C.c_int
        _lib.clip_host_face_polygon.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                                C.c_uint32, C.c_void_p]
    return _lib


def bbox_of(points: np.ndarray) -> np.ndarray:
    return np.concatenate([points.min(0), points.max(0)]).astype(np.float32)


def cell_geometry(points: np.ndarray, adjacency: np.ndarray, offsets: np.ndarray, cap: int = 256) -> dict:
    """The host build of the clipping core over every cell: what radfoam_amd.geometry.cell_geometry returns, as numpy,
    plus face_vertices and the per-cell status (0 ok, 1 a face outgrew ``cap`` vertices, 2 bad row)."""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    adj = np.ascontiguousarray(adjacency, dtype=np.uint32)
    off = np.ascontiguousarray(offsets, dtype=np.uint32)
    n, e = pts.shape[0], adj.shape[0]
    bbox = bbox_of(pts)
    out = dict(volume=np.empty(n), centroid=np.empty((n, 3)), bounded=np.empty(n, dtype=np.uint8),
               face_area=np.empty(e), face_vertices=np.empty(e, dtype=np.uint32), status=np.empty(n, dtype=np.uint32))
    out["bad"] = lib().clip_host_cell_geometry(pts.ctypes.data, n, adj.ctypes.data, off.ctypes.data, e, bbox.ctypes.data,
                                               cap, *(out[k].ctypes.data for k in (
                                                   "volume", "centroid", "bounded", "face_area", "face_vertices",
                                                   "status")))
    out["bounded"] = out["bounded"].astype(bool)
    return out


def face_polygon(points: np.ndarray, adjacency: np.ndarray, offsets: np.ndarray, a: int, slot: int, cap: int = 256):
    pts = np.ascontiguousarray(points, dtype=np.float32)
    adj = np.ascontiguousarray(adjacency, dtype=np.uint32)
    off = np.ascontiguousarray(offsets, dtype=np.uint32)
    bbox = bbox_of(pts)
    xyz = np.empty((cap, 3))
    m = lib().clip_host_face_polygon(pts.ctypes.data, adj.ctypes.data, off.ctypes.data, bbox.ctypes.data, a, slot, cap,
                                     xyz.ctypes.data)
    return None if m < 0 else xyz[:m].copy()


# ---- the reference: Qhull ------------------------------------------------------------------------------------------

def uniform_cloud(n: int = 1500, seed: int = 2) -> np.ndarray:
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(n, 3)).astype(np.float32)


def ring_cloud(seed: int = 5, k: int = 48, jitter: float = 1e-3) -> np.ndarray:
    """Two sites at (0,0,-+0.3) whose common face is a k-gon (48 by default): a ring of k sites at radius 1 (+-jitter)
    near z = 0 (+-jitter), and 400 sites on a radius-4 shell that close the cells."""
    rng = np.random.default_rng(seed)
    ang = 2.0 * np.pi * np.arange(k) / float(k)
    rad = 1.0 + rng.uniform(-jitter, jitter, k)
    ring = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-jitter, jitter, k)], axis=1)
    shell = rng.normal(size=(400, 3))
    shell *= 4.0 / np.linalg.norm(shell, axis=1, keepdims=True)
    return np.concatenate([[[0.0, 0.0, -0.3], [0.0, 0.0, 0.3]], ring, shell]).astype(np.float32)


def _shell(rng, count: int, radius: float) -> np.ndarray:
    s = rng.normal(size=(count, 3))
    return s * (radius / np.linalg.norm(s, axis=1, keepdims=True))


def hub_cloud(k: int, seed: int = 11) -> np.ndarray:
    """Site 0 at the origin, sites 1..k on a Fibonacci sphere of radius 1 jittered by +-1e-3 in every coordinate (all k
    are neighbours of site 0 and nothing else is: its row has exactly k entries), and 300 sites on a radius-4 shell that
    close the inner shell's cells.  Seed 11 meets the conditions tests/test_cell_geometry.py asserts for k = 64, 65, 200."""
    rng = np.random.default_rng(seed)
    i = np.arange(k) + 0.5
    z = 1.0 - 2.0 * i / k
    phi = np.pi * (1.0 + 5.0 ** 0.5) * i
    r = np.sqrt(1.0 - z * z)
    inner = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1) + rng.uniform(-1e-3, 1e-3, (k, 3))
    return np.concatenate([[[0.0, 0.0, 0.0]], inner, _shell(rng, 300, 4.0)]).astype(np.float32)


def clustered_cloud(seed: int = 3) -> np.ndarray:
    """600 sites: three Gaussian blobs of 150 with sigma 1, 1e-2 and 1e-4 (the box is [-1,1]^3, the blobs' centres uniform
    in its inner half) in a background of 150 sites uniform in [-4,4]^3.  Cell sizes span five orders of magnitude."""
    rng = np.random.default_rng(seed)
    blobs = [rng.normal(0.0, s, size=(150, 3)) + rng.uniform(-0.5, 0.5, 3) for s in (1.0, 1e-2, 1e-4)]
    return np.concatenate(blobs + [rng.uniform(-4.0, 4.0, size=(150, 3))]).astype(np.float32)


def grid_cloud(side: int = 6, spacing: float = 0.25) -> np.ndarray:
    """side^3 sites at spacing * (i, j, k) - 0.5, unjittered: site index (i * side + j) * side + k."""
    g = np.arange(side, dtype=np.float64) * spacing - 0.5
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)


REDO_SPREAD_PAIRS = ((0, 1), (2, 3), (72, 73), (200, 201))     # the axis sites of the four 17-rings


def redo_spread_cloud(seed: int = 7) -> np.ndarray:
    """Four 17-rings (ring_cloud's construction, jitter 1e-3) centred on (+-2, +-2, 0), inside 400 sites on a radius-9
    shell.  Their axis pairs sit at sites REDO_SPREAD_PAIRS: two pairs in the redo kernel's 64-cell block 0, one in block
    1, one in block 3; sites 4..71 are the ring sites, the rest the shell."""
    rng = np.random.default_rng(seed)
    axes, rings = [], []
    for cx, cy in ((-2.0, -2.0), (2.0, -2.0), (-2.0, 2.0), (2.0, 2.0)):
        ang = 2.0 * np.pi * np.arange(17) / 17.0
        rad = 1.0 + rng.uniform(-1e-3, 1e-3, 17)
        rings.append(np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang), rng.uniform(-1e-3, 1e-3, 17)], axis=1))
        axes.append(np.array([[cx, cy, -0.3], [cx, cy, 0.3]]))
    shell = _shell(rng, 400, 9.0)
    parts = [axes[0], axes[1]] + rings + [axes[2], shell[:126], axes[3], shell[126:]]
    pts = np.concatenate(parts).astype(np.float32)
    assert all(np.array_equal(pts[list(p)], axes[i].astype(np.float32)) for i, p in enumerate(REDO_SPREAD_PAIRS))
    return pts


def tiny_inputs() -> dict:
    """name -> (points, offsets, adjacency): 'n4' one tetrahedron (every cell open), 'n1' and 'n2' with an empty
    adjacency, 'empty_row' 60 uniform sites (seed 4) with Qhull's CSR from which the row of site EMPTY_ROW_SITE was
    taken out (the other rows still list it), and 'empty_row_full' the same before that."""
    from radfoam_amd import foam

    u32 = lambda x: np.asarray(x, dtype=np.uint32)
    tet = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
    out = {"n4": (tet, u32([0, 3, 6, 9, 12]), u32([1, 2, 3, 0, 2, 3, 0, 1, 3, 0, 1, 2])),
           "n1": (tet[:1], u32([0, 0]), u32([])), "n2": (tet[:2], u32([0, 0, 0]), u32([]))}
    pts = uniform_cloud(60, seed=4)
    off, adj = foam.delaunay_csr(pts)
    out["empty_row_full"] = (pts, off, adj)
    o = off.astype(np.int64)
    a = EMPTY_ROW_SITE
    cut = np.concatenate([o[:a + 1], o[a + 1:] - (o[a + 1] - o[a])])
    out["empty_row"] = (pts, u32(cut), np.concatenate([adj[:o[a]], adj[o[a + 1]:]]))
    return out


EMPTY_ROW_SITE = 8      # a bounded cell of that cloud


def cell_size(points: np.ndarray) -> float:
    """h = (bbox volume / N)^(1/3)"""
    ext = points.max(0).astype(np.float64) - points.min(0).astype(np.float64)
    return float((ext.prod() / points.shape[0]) ** (1.0 / 3.0))


def qhull_reference(points: np.ndarray) -> dict:
    """Per cell from scipy.spatial.Voronoi + ConvexHull of the region, in double: volume, centroid, and the two groups
    the tests use -- ``compared`` (Qhull-bounded, every vertex within one bbox diagonal of the bbox centre) and
    ``unbounded`` (Qhull reports the region open) -- plus ridge_vertices[(a, b)] = number of vertices of the face."""
    from scipy.spatial import ConvexHull, Voronoi

    p = points.astype(np.float64)
    n = p.shape[0]
    vor = Voronoi(p)
    lo, hi = p.min(0), p.max(0)
    centre, diag = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
    volume, centroid = np.full(n, np.nan), np.full((n, 3), np.nan)
    compared, unbounded = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for a in range(n):
        region = vor.regions[vor.point_region[a]]
        if len(region) == 0 or -1 in region:
            unbounded[a] = True
            continue
        verts = vor.vertices[region]
        if np.linalg.norm(verts - centre, axis=1).max() > diag:
            continue
        hull = ConvexHull(verts)
        # centroid of the hull: signed tetrahedra of its triangles about an interior point
        inner = verts.mean(0)
        tri = verts[hull.simplices] - inner
        vol6 = np.abs(np.einsum("ij,ij->i", tri[:, 0], np.cross(tri[:, 1], tri[:, 2])))
        volume[a] = vol6.sum() / 6.0
        centroid[a] = inner + (vol6[:, None] * tri.sum(1)).sum(0) / (4.0 * vol6.sum())
        compared[a] = True
    ridges = {}
    for (a, b), rv in zip(vor.ridge_points, vor.ridge_vertices):
        count = -1 if -1 in rv else len(rv)
        ridges[(int(a), int(b))] = ridges[(int(b), int(a))] = count
    return dict(volume=volume, centroid=centroid, compared=compared, unbounded=unbounded, ridge_vertices=ridges)


# ---- the cases and bars the CPU and GPU tests share ------------------------------------------------------------------

_CASES = {}

# seeds: ring* 5, hub* 11, clustered 3, the 400-site clouds 8 (seed 6 left 5.1 % of the bounded cells reaching past R / 2),
# redo_spread 7; each was checked against the conditions tests/test_cell_geometry.py asserts from the exact reference alone
_CLOUDS = {
    "uniform": uniform_cloud, "ring": ring_cloud,
    "ring16": lambda: ring_cloud(k=16), "ring17": lambda: ring_cloud(k=17),
    "ring256": lambda: ring_cloud(k=256, jitter=2e-5), "ring257": lambda: ring_cloud(k=257, jitter=2e-5),
    "hub64": lambda: hub_cloud(64), "hub65": lambda: hub_cloud(65), "hub200": lambda: hub_cloud(200),
    "clustered": clustered_cloud,
    "uniform400": lambda: uniform_cloud(400, seed=8),
    "offset": lambda: (uniform_cloud(400, seed=8) + np.array([1000.0, -2000.0, 500.0], dtype=np.float32)),
    "scaled_small": lambda: uniform_cloud(400, seed=8) * np.float32(2.0 ** -10),
    "scaled_large": lambda: uniform_cloud(400, seed=8) * np.float32(2.0 ** 10),
    "grid": grid_cloud, "redo_spread": redo_spread_cloud,
}


def case(name: str) -> dict:
    """A named cloud (_CLOUDS): points, Qhull's CSR, rows and h; computed once per process and never modified.
    'uniform' (N = 1500, seed 2) and 'ring' (the 48-gon) carry the Qhull reference ``ref``; every other case carries
    the exact reference instead (tests/cell_geometry_ref.py): ``exact``, its faces per adjacency slot ``slots``, and
    R = 4 |bbox diagonal| as the kernel takes it."""
    if name not in _CASES:
        from radfoam_amd import foam

        pts = _CLOUDS[name]()
        assert pts.dtype == np.float32
        off, adj = foam.delaunay_csr(pts)
        c = dict(points=pts, offsets=off, adjacency=adj, h=cell_size(pts),
                 rows=np.repeat(np.arange(pts.shape[0]), np.diff(off.astype(np.int64))))
        if name in ("uniform", "ring"):
            c["ref"] = qhull_reference(pts)
        else:
            from tests import cell_geometry_ref as X

            c["exact"] = X.exact_geometry(pts)
            c["slots"] = X.per_slot(c["exact"], off, adj)
            bb = bbox_of(pts).astype(np.float64)
            c["R"] = 4.0 * float(np.sqrt(((bb[3:] - bb[:3]) ** 2).sum()))
        _CASES[name] = c
    return _CASES[name]


def slot_of(c: dict, a: int, b: int) -> int:
    """the adjacency slot of b in a's row"""
    lo, hi = int(c["offsets"][a]), int(c["offsets"][a + 1])
    e = lo + int(np.searchsorted(c["adjacency"][lo:hi], b))
    assert e < hi and c["adjacency"][e] == b
    return e


def _check_cells_local(c, volume, centroid, bounded, eps, share, cells):
    ex, R = c["exact"], c["R"]
    open_ = ex["open"]
    must = ~open_ & (ex["extent"] < 0.5 * R)
    either = ~open_ & ~must
    print(f"cells {open_.size}: open {open_.sum()}, must be bounded {must.sum()}, either way {either.sum()} "
          f"({100.0 * either.sum() / max(1, (~open_).sum()):.2f} % of the bounded)")
    assert not bounded[open_].any() and np.isposinf(volume[open_]).all() and np.isnan(centroid[open_]).all()
    assert bounded[must].all()
    if share is not None:
        assert either.sum() <= share * (~open_).sum()
    assert np.isfinite(volume[bounded]).all() and np.isfinite(centroid[bounded]).all()
    assert np.isposinf(volume[~bounded]).all() and np.isnan(centroid[~bounded]).all()
    cmp_ = ~open_ & bounded
    if cells is not None:
        pick = np.zeros_like(cmp_)
        pick[cells] = True
        assert cmp_[pick].all()
        cmp_ = pick
    s = np.cbrt(ex["volume_f"][cmp_])
    rv = (np.abs(volume[cmp_] - ex["volume_f"][cmp_]) / s ** 3).max()
    rc = (np.abs(centroid[cmp_] - ex["centroid_f"][cmp_]).max(1) / s).max()
    print(f"compared {cmp_.sum()}: max |dV| / s^3 = {rv:.3g}, max |dc| / s = {rc:.3g} (bar {eps:.3g})")
    assert rv <= eps and rc <= eps
    return rv, rc


def check_cells(c: dict, volume, centroid, bounded, local: bool = False, eps: float = 1e-9, share=0.05, cells=None):
    """Test 1 of the cell geometry: on Qhull's compared set bounded, |V - V_ref| <= 1e-9 h^3, |c - c_ref| <= 1e-9 h;
    every Qhull-unbounded cell unbounded with volume +inf (and centroid NaN); cells in neither group may go either way,
    consistently.

    ``local``: against the exact reference of the case and in units of each cell's own size s_a = V_ref,a^(1/3):
    |V - V_ref| <= eps s_a^3 and |c - c_ref| <= eps s_a on every cell the reference calls bounded (and the code did not
    call open, which it may only where the cell reaches past R / 2), or on ``cells`` alone, which must all be among
    them.  Every open cell must come out open, every bounded cell whose faces stay within R / 2 of their centres
    bounded, and the cells that may go either way are at most ``share`` of the bounded ones (None: printed only).
    Returns the two worst ratios."""
    if local:
        return _check_cells_local(c, volume, centroid, bounded, eps, share, cells)
    ref, h = c["ref"], c["h"]
    cmp_, unb = ref["compared"], ref["unbounded"]
    assert bounded[cmp_].all()
    dv = np.abs(volume[cmp_] - ref["volume"][cmp_]).max()
    dc = np.abs(centroid[cmp_] - ref["centroid"][cmp_]).max()
    print(f"compared {cmp_.sum()} of {cmp_.size}: max |dV| = {dv / h ** 3:.3g} h^3, max |dc| = {dc / h:.3g} h")
    assert dv <= 1e-9 * h ** 3 and dc <= 1e-9 * h
    assert not bounded[unb].any() and np.isposinf(volume[unb]).all() and np.isnan(centroid[unb]).all()
    assert np.isfinite(volume[bounded]).all() and np.isfinite(centroid[bounded]).all()
    assert np.isposinf(volume[~bounded]).all() and np.isnan(centroid[~bounded]).all()


def check_faces(c: dict, volume, bounded, face_area, local: bool = False, eps: float = 1e-9):
    """Test 2: on pairs of bounded cells area(a->b) == area(b->a); per bounded cell the area vectors close and
    volume == sum area |d_b| / 6; all to 1e-9 h^2 (h^3 for the volume).

    ``local``: the same identities in units of each cell's own size s_a (the reference's; the smaller cell's for a
    pair), to ``eps``; and every face the exact reference calls bounded and within R / 2 of its centre has a finite area
    within eps min(s_a, s_b)^2 of the reference's.  Returns the four worst ratios."""
    pts, adj, rows = c["points"].astype(np.float64), c["adjacency"].astype(np.int64), c["rows"]
    n = pts.shape[0]
    if local:
        size = np.cbrt(c["exact"]["volume_f"])                  # +inf for an open cell
        size = np.where(bounded | ~c["exact"]["open"], size, np.inf)
        assert np.isfinite(size[bounded]).all()
        pair = np.minimum(size[rows], size[adj])
    else:
        size = np.full(n, c["h"])
        pair = size[rows]
    key = rows * n + adj
    order = np.argsort(key)
    back = order[np.searchsorted(key[order], adj * n + rows)]          # the slot of (b -> a)
    assert (adj[back] == rows).all() and (rows[back] == adj).all()
    both = bounded[rows] & bounded[adj]
    sym = (np.abs(face_area[both] - face_area[back][both]) / pair[both] ** 2).max() if both.any() else 0.0
    of_bounded = bounded[rows]
    assert np.isfinite(face_area[of_bounded]).all()
    d = pts[adj] - pts[rows]
    length = np.linalg.norm(d, axis=1)
    with np.errstate(invalid="ignore"):      # inf * 0 on the faces of unbounded cells, which the where() drops
        vec = np.where(of_bounded[:, None], face_area[:, None] * d / length[:, None], 0.0)
    closed = np.zeros((n, 3))
    np.add.at(closed, rows, vec)
    vol = np.zeros(n)
    np.add.at(vol, rows, np.where(of_bounded, face_area * length / 6.0, 0.0))
    gap = (np.linalg.norm(closed[bounded], axis=1) / size[bounded] ** 2).max() if bounded.any() else 0.0
    dvol = (np.abs(vol[bounded] - volume[bounded]) / size[bounded] ** 3).max() if bounded.any() else 0.0
    unit = "s" if local else "h"
    print(f"faces: symmetry {sym:.3g} {unit}^2, closure {gap:.3g} {unit}^2, volume identity {dvol:.3g} {unit}^3")
    assert sym <= eps and gap <= eps and dvol <= eps
    if not local:
        return sym, gap, dvol
    slots = c["slots"]
    cmp_ = np.isfinite(slots["area"]) & (slots["extent"] < 0.5 * c["R"]) & np.isfinite(pair)
    assert np.isfinite(face_area[cmp_]).all() and not np.isnan(face_area).any()
    da = (np.abs(face_area[cmp_] - slots["area"][cmp_]) / pair[cmp_] ** 2).max() if cmp_.any() else 0.0
    print(f"faces compared {cmp_.sum()} of {cmp_.size}: max |dA| / s^2 = {da:.3g} (bar {eps:.3g})")
    assert da <= eps
    return sym, gap, dvol, da


# ---- what the CPU and GPU tests of the exact-reference cases share -----------------------------------------------------

GRID_H = 0.25


def check_against_exact(c: dict, out: dict, share=0.05, cells=None, vertices: bool = True, eps: float = 1e-9):
    """``out``: volume, centroid, bounded, face_area, face_vertices as numpy.  check_cells and check_faces in their
    per-cell-scale mode, and the polygons have the reference's distinct-vertex counts wherever both cells are bounded."""
    worst = check_cells(c, out["volume"], out["centroid"], out["bounded"], local=True, eps=eps, share=share, cells=cells)
    worst += check_faces(c, out["volume"], out["bounded"], out["face_area"], local=True, eps=eps)
    if vertices:
        both = out["bounded"][c["rows"]] & out["bounded"][c["adjacency"]]
        assert np.array_equal(out["face_vertices"][both].astype(np.int64), c["slots"]["vertices"][both])
    return worst


def grid_interior(side: int = 6) -> np.ndarray:
    i = np.arange(side)
    inner = (i >= 1) & (i <= side - 2)
    return (inner[:, None, None] & inner[None, :, None] & inner[None, None, :]).reshape(-1)


def check_grid(c: dict, out: dict, eps: float = 1e-9):
    """The closed form on the unjittered grid: interior cells have volume h^3 and the centroid at the site, their six
    axis faces area h^2, every other listed face of theirs area <= eps h^2; nothing is NaN."""
    h, pts = GRID_H, c["points"].astype(np.float64)
    inner = grid_interior()
    assert np.array_equal(inner, ~c["exact"]["open"]) and out["bounded"][inner].all()
    dv = np.abs(out["volume"][inner] - h ** 3).max() / h ** 3
    dc = np.abs(out["centroid"][inner] - pts[inner]).max() / h
    rows, adj = c["rows"], c["adjacency"].astype(np.int64)
    of_inner = inner[rows]
    axis = of_inner & (np.abs(np.abs(pts[adj] - pts[rows]).sum(1) - h) == 0.0)         # an axis neighbour: |d|_1 == h
    assert (np.bincount(rows[axis], minlength=len(pts))[inner] == 6).all()
    assert not np.isnan(out["face_area"]).any() and np.isfinite(out["face_area"][of_inner]).all()
    da = np.abs(out["face_area"][axis] - h * h).max() / h ** 2
    dz = np.abs(out["face_area"][of_inner & ~axis]).max() / h ** 2
    print(f"grid: |dV| {dv:.3g} h^3, |dc| {dc:.3g} h, axis faces {da:.3g} h^2, zero faces {dz:.3g} h^2 "
          f"({(of_inner & ~axis).sum()} of them)")
    assert (of_inner & ~axis).sum() > 0
    assert dv <= eps and dc <= eps and da <= eps and dz <= eps


def check_surface(c: dict, inside: np.ndarray, tri: np.ndarray, edge: np.ndarray, volume: float, scale: float,
                  area=None, eps: float = 1e-9, counts: bool = True):
    """A cell_surface answer: triangles only from straddling slots in slot order, no NaN corner, Sum (reference face
    vertices - 2) triangles per slot (``counts``), |enclosed volume - volume| <= eps scale^3 (and |area - ``area``| <= eps scale^2)."""
    rows, adj = c["rows"], c["adjacency"].astype(np.int64)
    straddle = inside[rows] & ~inside[adj]
    assert tri.shape == (len(edge), 3, 3) and not np.isnan(tri).any()
    assert straddle[edge].all() and (np.diff(edge) >= 0).all()
    if counts:
        want = np.maximum(c["slots"]["vertices"][straddle] - 2, 0)
        assert np.array_equal(np.bincount(edge, minlength=len(adj))[straddle], want) and len(edge) == want.sum()
    enclosed = np.einsum("ij,ij->i", tri[:, 0], np.cross(tri[:, 1], tri[:, 2])).sum() / 6.0
    total = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1).sum()
    print(f"surface: {len(edge)} triangles, |enclosed - V| = {abs(enclosed - volume) / scale ** 3:.3g} s^3, area "
          f"{total / scale ** 2:.6g} s^2")
    assert abs(enclosed - volume) <= eps * scale ** 3
    if area is not None:
        assert abs(total - area) <= eps * scale ** 2


def host_surface(c: dict, inside: np.ndarray):
    """cell_surface through the host build: the fan of face_polygon for every straddling slot of three or more
    vertices (what surface_count_kernel / surface_emit_kernel do on the device)."""
    rows, adj = c["rows"], c["adjacency"].astype(np.int64)
    tri, edge = [], []
    for e in np.nonzero(inside[rows] & ~inside[adj])[0]:
        poly = face_polygon(c["points"], c["adjacency"], c["offsets"], int(rows[e]), int(e))
        for k in range(1, len(poly) - 1):
            tri.append([poly[0], poly[k], poly[k + 1]])
            edge.append(int(e))
    return np.array(tri).reshape(-1, 3, 3), np.array(edge, dtype=np.int64)
