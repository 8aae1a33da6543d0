"""ctypes loader of the HOST build of radfoam_amd/csrc/rf_clip.hpp (test harness; see clip_host.cpp), and the Qhull
reference the cell-geometry tests compare against (scipy.spatial.Voronoi + ConvexHull per region, in double)."""
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


def ring_cloud(seed: int = 5) -> np.ndarray:
    """Two sites at (0,0,-+0.3) whose common face is a 48-gon: a ring of 48 sites at radius 1 (+-1e-3) near z = 0
    (+-1e-3), and 400 sites on a radius-4 shell that close the cells."""
    rng = np.random.default_rng(seed)
    ang = 2.0 * np.pi * np.arange(48) / 48.0
    rad = 1.0 + rng.uniform(-1e-3, 1e-3, 48)
    ring = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-1e-3, 1e-3, 48)], axis=1)
    shell = rng.normal(size=(400, 3))
    shell *= 4.0 / np.linalg.norm(shell, axis=1, keepdims=True)
    return np.concatenate([[[0.0, 0.0, -0.3], [0.0, 0.0, 0.3]], ring, shell]).astype(np.float32)


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


def case(name: str) -> dict:
    """'uniform' (N = 1500, seed 2) or 'ring' (the 48-gon): points, Qhull's CSR, the Qhull reference and h; computed
    once per process and never modified."""
    if name not in _CASES:
        from radfoam_amd import foam

        pts = uniform_cloud() if name == "uniform" else ring_cloud()
        off, adj = foam.delaunay_csr(pts)
        _CASES[name] = dict(points=pts, offsets=off, adjacency=adj, ref=qhull_reference(pts), h=cell_size(pts),
                            rows=np.repeat(np.arange(pts.shape[0]), np.diff(off.astype(np.int64))))
    return _CASES[name]


def check_cells(c: dict, volume, centroid, bounded):
    """Test 1 of the cell geometry: on Qhull's compared set bounded, |V - V_ref| <= 1e-9 h^3, |c - c_ref| <= 1e-9 h;
    every Qhull-unbounded cell unbounded with volume +inf (and centroid NaN); cells in neither group may go either way,
    consistently."""
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


def check_faces(c: dict, volume, bounded, face_area):
    """Test 2: on pairs of bounded cells area(a->b) == area(b->a); per bounded cell the area vectors close and
    volume == sum area |d_b| / 6; all to 1e-9 h^2 (h^3 for the volume)."""
    pts, adj, rows, h = c["points"].astype(np.float64), c["adjacency"].astype(np.int64), c["rows"], c["h"]
    n = pts.shape[0]
    key = rows * n + adj
    order = np.argsort(key)
    back = order[np.searchsorted(key[order], adj * n + rows)]          # the slot of (b -> a)
    assert (adj[back] == rows).all() and (rows[back] == adj).all()
    both = bounded[rows] & bounded[adj]
    sym = np.abs(face_area[both] - face_area[back][both]).max()
    of_bounded = bounded[rows]
    assert np.isfinite(face_area[of_bounded]).all()
    d = pts[adj] - pts[rows]
    length = np.linalg.norm(d, axis=1)
    vec = np.where(of_bounded[:, None], face_area[:, None] * d / length[:, None], 0.0)
    closed = np.zeros((n, 3))
    np.add.at(closed, rows, vec)
    vol = np.zeros(n)
    np.add.at(vol, rows, np.where(of_bounded, face_area * length / 6.0, 0.0))
    gap = np.linalg.norm(closed[bounded], axis=1).max()
    dvol = np.abs(vol[bounded] - volume[bounded]).max()
    print(f"faces: symmetry {sym / h ** 2:.3g} h^2, closure {gap / h ** 2:.3g} h^2, volume identity {dvol / h ** 3:.3g} h^3")
    assert sym <= 1e-9 * h ** 2 and gap <= 1e-9 * h ** 2 and dvol <= 1e-9 * h ** 3
