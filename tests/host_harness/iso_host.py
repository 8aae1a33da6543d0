"""ctypes loader of the HOST build of radfoam_amd/csrc/rf_iso.hpp (test harness; see iso_host.cpp), the welded mesh put
together from it the way radfoam_amd/isosurface.py does on the device, and the clouds and checks the CPU and GPU tests of
isosurface share."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libiso_host.so")
_SRC = [os.path.join(_HERE, "iso_host.cpp"), os.path.join(_HERE, "..", "..", "radfoam_amd", "csrc", "rf_iso.hpp")]


def build():
    if os.path.exists(_SO) and all(os.path.getmtime(s) <= os.path.getmtime(_SO) for s in _SRC):
        return _SO
    os.makedirs(os.path.dirname(_SO), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", _SO, _SRC[0]], check=True)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        P, U = C.c_void_p, C.c_uint32
        _lib.iso_host_count.restype = C.c_int64
        _lib.iso_host_count.argtypes = [P, U, P, U, C.c_double, P]
        _lib.iso_host_emit.restype = None
        _lib.iso_host_emit.argtypes = [P, U, P, P, U, C.c_double, P, P, P]
        _lib.iso_host_vertices.restype = None
        _lib.iso_host_vertices.argtypes = [P, P, U, P, U, C.c_double, P, P]
        _lib.iso_host_vertices_grad.restype = None
        _lib.iso_host_vertices_grad.argtypes = [P, P, U, P, U, C.c_double, P, P]
    return _lib


def _field(points, values):
    pts = np.ascontiguousarray(points, dtype=np.float32)
    val = np.ascontiguousarray(values, dtype=np.float32)
    assert pts.ndim == 2 and pts.shape[1] == 3 and val.shape == (pts.shape[0],)
    return pts, val


def extract(points, tets, values, level):
    """(counts u8[T], keys int64[F,3], triangle_tet int64[F], the first tetrahedron out of range or -1)"""
    pts, val = _field(points, values)
    tt = np.ascontiguousarray(tets, dtype=np.int64).reshape(-1, 4)
    counts = np.zeros(tt.shape[0], dtype=np.uint8)
    bad = lib().iso_host_count(tt.ctypes.data, tt.shape[0], val.ctypes.data, pts.shape[0], level, counts.ctypes.data)
    nf = int(counts.sum())
    keys, tri_tet = np.full((nf, 3), -7, dtype=np.int64), np.full(nf, -7, dtype=np.int64)
    lib().iso_host_emit(tt.ctypes.data, tt.shape[0], pts.ctypes.data, val.ctypes.data, pts.shape[0], level,
                        counts.ctypes.data, keys.ctypes.data, tri_tet.ctypes.data)
    return counts, keys, tri_tet, int(bad)


def vertices(points, values, vertex_sites, level):
    """(x f64[V,3], t f64[V])"""
    pts, val = _field(points, values)
    sites = np.ascontiguousarray(vertex_sites, dtype=np.int64).reshape(-1, 2)
    x, t = np.empty((sites.shape[0], 3)), np.empty(sites.shape[0])
    lib().iso_host_vertices(pts.ctypes.data, val.ctypes.data, pts.shape[0], sites.ctypes.data, sites.shape[0], level,
                            x.ctypes.data, t.ctypes.data)
    return x, t


def vertices_grad(points, values, vertex_sites, level, grad_vertices) -> np.ndarray:
    """f64[V,2,4]: what every vertex gives (p_a, v_a) and (p_b, v_b)"""
    pts, val = _field(points, values)
    sites = np.ascontiguousarray(vertex_sites, dtype=np.int64).reshape(-1, 2)
    g = np.ascontiguousarray(grad_vertices, dtype=np.float64)
    assert g.shape == (sites.shape[0], 3)
    out = np.empty((sites.shape[0], 2, 4))
    lib().iso_host_vertices_grad(pts.ctypes.data, val.ctypes.data, pts.shape[0], sites.ctypes.data, sites.shape[0], level,
                                 g.ctypes.data, out.ctypes.data)
    return out


def mesh(points, tets, values, level) -> dict:
    """The IsoMesh of radfoam.isosurface as numpy from the host build: one vertex per distinct key, rows ascending"""
    _, keys, tri_tet, bad = extract(points, tets, values, level)
    assert bad < 0
    uniq, inverse = np.unique(keys.reshape(-1), return_inverse=True)
    sites = np.stack([uniq >> 32, uniq & 0xFFFFFFFF], 1).astype(np.int64).reshape(-1, 2)
    x, t = vertices(points, values, sites, level)
    return dict(vertices=x, vertex_sites=sites, vertex_t=t, triangles=inverse.reshape(-1, 3).astype(np.int64),
                triangle_tet=tri_tet)


# ---- the clouds -------------------------------------------------------------------------------------------------------

RADIUS = 0.6
# (n, seed) -> (tetrahedra, V, F) of values = RADIUS - |p| at level 0, counted when the feature was proposed
CLOUDS = {(64, 0): (295, 82, 160), (400, 1): (2432, 322, 640), (400, 2): (2424, 273, 542), (1000, 3): (6263, 565, 1126)}
_CLOUD = {}


def cloud(n: int, seed: int) -> dict:
    """points f32[n,3] uniform in [-1,1)^3, their Delaunay tetrahedra int64[T,4] (scipy) and the ball's field, once"""
    if (n, seed) not in _CLOUD:
        from scipy.spatial import Delaunay

        pts = np.random.default_rng(seed).uniform(-1, 1, (n, 3)).astype(np.float32)
        tets = np.ascontiguousarray(Delaunay(pts.astype(np.float64)).simplices, dtype=np.int64)
        values = (RADIUS - np.linalg.norm(pts.astype(np.float64), axis=1)).astype(np.float32)
        _CLOUD[(n, seed)] = dict(points=pts, tets=tets, values=values)
    return _CLOUD[(n, seed)]


def mask_pair():
    """(points f32[4,3], tets int64[2,4]): one positively and one negatively oriented tetrahedron on the same sites"""
    pts = np.array([[0.1, 0.0, -0.2], [1.0, 0.2, 0.1], [-0.1, 0.9, 0.0], [0.2, 0.1, 1.1]], dtype=np.float32)
    return pts, np.array([[0, 1, 2, 3], [0, 2, 1, 3]], dtype=np.int64)


def mask_values(mask: int, level: float) -> np.ndarray:
    """f32[4]: site c above the level where bit c of mask is set, all at different distances from it"""
    offsets = np.array([0.3, 0.7, 0.45, 0.9])
    return np.where([(mask >> c) & 1 for c in range(4)], level + offsets, level - offsets[::-1]).astype(np.float32)


def write_arrays(which, path):
    """The plain arrays tests/host_harness/iso_sanitize.cpp reads: ``which`` is "masks" (the pair of tetrahedra under all
    sixteen masks at level 0.25) or an (n, seed) of CLOUDS (the ball's field at level 0)."""
    if which == "masks":
        pts, tets = mask_pair()
        fields = [(0.25, mask_values(mask, 0.25)) for mask in range(16)]
    else:
        c = cloud(*which)
        pts, tets, fields = c["points"], c["tets"], [(0.0, c["values"])]
    with open(path, "wb") as f:
        np.array([len(pts), len(tets), len(fields)], dtype=np.uint32).tofile(f)
        np.ascontiguousarray(pts, dtype=np.float32).tofile(f)
        np.ascontiguousarray(tets, dtype=np.int64).tofile(f)
        for level, values in fields:
            np.array([level], dtype=np.float64).tofile(f)
            np.ascontiguousarray(values, dtype=np.float32).tofile(f)


# ---- what the CPU and GPU tests share ----------------------------------------------------------------------------------

def check_closed(mesh: dict, label: str = ""):
    """Closed and oriented (every directed edge once, its reverse once) and V - E + F = 2.  Returns (V, E, F)."""
    tri, nv = np.asarray(mesh["triangles"]), len(mesh["vertices"])
    assert len(tri) and tri.min() >= 0 and tri.max() < nv and len(np.unique(tri)) == nv
    u, w = tri.reshape(-1), tri[:, [1, 2, 0]].reshape(-1)
    assert (u != w).all()
    code = u * nv + w
    assert len(np.unique(code)) == len(code), "a directed edge occurs twice"
    assert np.array_equal(np.sort(w * nv + u), np.sort(code)), "a directed edge has no mate"
    ne, nf = len(code) // 2, len(tri)
    assert nv - ne + nf == 2, f"V - E + F = {nv} - {ne} + {nf}"
    print(f"{label}: V {nv}, E {ne}, F {nf}: closed, oriented, V - E + F = 2")
    return nv, ne, nf


def enclosed_volume(mesh: dict) -> float:
    """by the divergence theorem: the sum of the signed volumes of (origin, triangle)"""
    x = np.asarray(mesh["vertices"])[np.asarray(mesh["triangles"])]
    return float(np.einsum("fi,fi->f", x[:, 0], np.cross(x[:, 1], x[:, 2])).sum() / 6.0)


def area_vectors(mesh: dict, num_tets: int) -> np.ndarray:
    """f64[T,3]: the sum of the area vectors of every tetrahedron's triangles"""
    x = np.asarray(mesh["vertices"])[np.asarray(mesh["triangles"])]
    out = np.zeros((num_tets, 3))
    np.add.at(out, np.asarray(mesh["triangle_tet"]), 0.5 * np.cross(x[:, 1] - x[:, 0], x[:, 2] - x[:, 0]))
    return out


def key_sets(mesh: dict, num_tets: int) -> list:
    """per tetrahedron the set of its triangles' keys (a, b)"""
    sites, tri, tet = np.asarray(mesh["vertex_sites"]), np.asarray(mesh["triangles"]), np.asarray(mesh["triangle_tet"])
    out = [set() for _ in range(num_tets)]
    for f in range(len(tri)):
        out[tet[f]].update(tuple(sites[v]) for v in tri[f])
    return out
