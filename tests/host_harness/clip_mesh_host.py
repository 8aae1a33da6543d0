"""ctypes loader of the HOST build of radfoam_amd/csrc/rf_clip_mesh.hpp (test harness; see clip_mesh_host.cpp), the
welded mesh put together from it the way radfoam_amd/mesh.py does on the device, and the checks the CPU and GPU tests of
cell_mesh share."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from tests.host_harness import clip_host as H

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libclip_mesh_host.so")
_CSRC = os.path.join(_HERE, "..", "..", "radfoam_amd", "csrc")
_SRC = [os.path.join(_HERE, "clip_mesh_host.cpp"), os.path.join(_CSRC, "rf_clip_mesh.hpp"),
        os.path.join(_CSRC, "rf_clip_area_grad.hpp"), os.path.join(_CSRC, "rf_clip.hpp")]
NO_SITE = 0xFFFFFFFF


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
        _lib.clip_mesh_host_face_count.restype = C.c_int
        _lib.clip_mesh_host_face_count.argtypes = [C.c_void_p] * 4 + [C.c_uint32] * 3
        _lib.clip_mesh_host_face_corners.restype = C.c_int
        _lib.clip_mesh_host_face_corners.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                                     C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p] * 2
        _lib.clip_mesh_host_vertices.restype = None
        _lib.clip_mesh_host_vertices.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
        _lib.clip_mesh_host_vertices_grad.restype = None
        _lib.clip_mesh_host_vertices_grad.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                                      C.c_void_p]
    return _lib


def _arrays(points, adjacency, offsets):
    pts = np.ascontiguousarray(points, dtype=np.float32)
    adj = np.ascontiguousarray(adjacency, dtype=np.uint32)
    off = np.ascontiguousarray(offsets, dtype=np.uint32)
    return pts, adj, off, H.bbox_of(pts)


def face_count(points, adjacency, offsets, a: int, slot: int, cap: int = 256) -> int:
    pts, adj, off, bbox = _arrays(points, adjacency, offsets)
    return lib().clip_mesh_host_face_count(pts.ctypes.data, adj.ctypes.data, off.ctypes.data, bbox.ctypes.data, a, slot, cap)


def face_corners(points, adjacency, offsets, a: int, slot: int, expect: int, cap: int = 256):
    """(status, xyz f64[expect,3], sites u32[expect,4]) of rf::clip::face_corners_serial"""
    pts, adj, off, bbox = _arrays(points, adjacency, offsets)
    xyz, sites = np.full((expect, 3), -1.0), np.zeros((expect, 4), dtype=np.uint32)
    status = lib().clip_mesh_host_face_corners(pts.ctypes.data, pts.shape[0], adj.ctypes.data, off.ctypes.data, adj.shape[0],
                                               bbox.ctypes.data, a, slot, cap, expect, xyz.ctypes.data, sites.ctypes.data)
    return status, xyz, sites


def vertices(points, vertex_sites) -> np.ndarray:
    pts = np.ascontiguousarray(points, dtype=np.float32)
    keys = np.ascontiguousarray(vertex_sites, dtype=np.int64).reshape(-1, 4)
    out = np.empty((keys.shape[0], 3))
    lib().clip_mesh_host_vertices(pts.ctypes.data, pts.shape[0], keys.ctypes.data, keys.shape[0], out.ctypes.data)
    return out


def vertices_grad(points, vertex_sites, grad_vertices) -> np.ndarray:
    """f64[V,4,3]: what every vertex gives its four sites"""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    keys = np.ascontiguousarray(vertex_sites, dtype=np.int64).reshape(-1, 4)
    g = np.ascontiguousarray(grad_vertices, dtype=np.float64)
    assert g.shape == (keys.shape[0], 3)
    out = np.empty((keys.shape[0], 4, 3))
    lib().clip_mesh_host_vertices_grad(pts.ctypes.data, pts.shape[0], keys.ctypes.data, keys.shape[0], g.ctypes.data,
                                       out.ctypes.data)
    return out


# ---- the selections and the mesh --------------------------------------------------------------------------------------

# name -> (cloud of clip_host.case, the cells asked for); bounded cells only
SELECTIONS = {"uniform400": lambda p: np.linalg.norm(p, axis=1) < 0.6, "uniform": lambda p: np.linalg.norm(p, axis=1) < 0.6,
              "clustered": lambda p: np.linalg.norm(p, axis=1) < 2.0}
# F, C, V, largest polygon of those selections, counted from the serial routine when the feature was proposed
TABLE = {"uniform400": (348, 1752, 530, 10), "uniform": (674, 3398, 1027, 11), "hub64": (64, 372, 124, 6),
         "hub65": (65, 378, 126, 6), "ring16": (52, 300, 100, 16), "ring17": (49, 282, 94, 17),
         "clustered": (330, 1656, 500, 11)}

_HOST = {}


def host_geometry(name: str) -> dict:
    key = ("geometry", name)
    if key not in _HOST:
        c = H.case(name)
        _HOST[key] = H.cell_geometry(c["points"], c["adjacency"], c["offsets"])
        assert _HOST[key]["bad"] == 0
    return _HOST[key]


def selection(name: str) -> np.ndarray:
    """bool[N]: the cells of the named selection; the grid's 64 interior cells, cell 0 of the hubs and rings, and the
    bounded cells whose site is within the ball for the rest"""
    c = H.case(name)
    if name == "grid":
        return H.grid_interior()
    if name in SELECTIONS:
        return SELECTIONS[name](c["points"].astype(np.float64)) & host_geometry(name)["bounded"]
    inside = np.zeros(c["points"].shape[0], dtype=bool)
    inside[0] = True
    assert host_geometry(name)["bounded"][0]
    return inside


def weld(slots, counts, xyz, sites) -> dict:
    """The mesh of radfoam.cell_mesh as numpy from the corners of the listed faces (in slot order): one vertex per
    distinct key, rows ascending, positioned by the lowest-numbered corner that carries the key."""
    slots, counts = np.asarray(slots, dtype=np.int64), np.asarray(counts, dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    keys = sites.astype(np.int64).reshape(-1, 4)
    if keys.shape[0]:
        vertex_sites, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
        inverse = inverse.reshape(-1)
    else:
        vertex_sites, first, inverse = keys, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    tri, tri_slot = [], []
    for f in range(len(slots)):
        v = inverse[offsets[f]:offsets[f + 1]]
        for k in range(1, len(v) - 1):
            tri.append((v[0], v[k], v[k + 1]))
            tri_slot.append(slots[f])
    return dict(vertices=xyz.reshape(-1, 3)[first], vertex_sites=vertex_sites, polygon_offsets=offsets,
                polygon_vertices=inverse.astype(np.int64), polygon_slot=slots,
                triangles=np.array(tri, dtype=np.int64).reshape(-1, 3), triangle_slot=np.array(tri_slot, dtype=np.int64),
                corner_xyz=xyz.reshape(-1, 3), corner_sites=keys)


def host_mesh(name: str) -> dict:
    """weld() of the serial routine's corners over the named selection, once per process; ``counts`` are the serial
    routine's own vertex counts (face_count), which face_corners is then held to."""
    key = ("mesh", name)
    if key not in _HOST:
        c, inside = H.case(name), selection(name)
        rows, adj = c["rows"], c["adjacency"].astype(np.int64)
        slots, counts, xyz, sites = [], [], [], []
        for e in np.nonzero(inside[rows] & ~inside[adj])[0]:
            m = face_count(c["points"], c["adjacency"], c["offsets"], int(rows[e]), int(e))
            assert m >= 0
            if m < 3:
                continue
            status, x, s = face_corners(c["points"], c["adjacency"], c["offsets"], int(rows[e]), int(e), m)
            assert status == 0
            slots.append(int(e)), counts.append(m), xyz.append(x), sites.append(s)
        xyz = np.concatenate(xyz) if xyz else np.zeros((0, 3))
        sites = np.concatenate(sites) if sites else np.zeros((0, 4), dtype=np.uint32)
        _HOST[key] = dict(weld(slots, counts, xyz, sites), inside=inside)
    return _HOST[key]


# ---- what the CPU and GPU tests share ----------------------------------------------------------------------------------

def check_topology(mesh: dict, label: str = ""):
    """Closed and oriented (every directed edge once, its reverse once), no vertex twice in a polygon, and
    V - E + F = 2 on every connected component.  Returns (V, E, F, components)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    off, pv = np.asarray(mesh["polygon_offsets"]), np.asarray(mesh["polygon_vertices"])
    nv, nf = len(mesh["vertices"]), len(off) - 1
    assert nf > 0 and off[0] == 0 and off[-1] == len(pv) and (np.diff(off) >= 3).all()
    assert pv.min() >= 0 and pv.max() < nv and len(np.unique(pv)) == nv
    poly = np.repeat(np.arange(nf), np.diff(off))
    nxt = np.arange(len(pv)) + 1
    nxt[off[1:] - 1] = off[:-1]
    for f in range(nf):
        v = pv[off[f]:off[f + 1]]
        assert len(np.unique(v)) == len(v), f"polygon {f} repeats a vertex"
    u, w = pv, pv[nxt]
    code = u * nv + w
    assert len(np.unique(code)) == len(code), "a directed edge occurs twice"
    assert np.array_equal(np.sort(w * nv + u), np.sort(code)), "a directed edge has no mate"
    ncomp, comp = connected_components(coo_matrix((np.ones(len(u)), (u, w)), shape=(nv, nv)), directed=False)
    for k in range(ncomp):
        vk, ek, fk = int((comp == k).sum()), int((comp[u] == k).sum()) // 2, len(np.unique(poly[comp[u] == k]))
        assert vk - ek + fk == 2, f"component {k}: V - E + F = {vk} - {ek} + {fk}"
    print(f"{label}: V {nv}, E {len(u) // 2}, F {nf}, components {ncomp}: closed, oriented, V - E + F = 2 each")
    return nv, len(u) // 2, nf, ncomp


def check_fans(mesh: dict):
    """triangles / triangle_slot are the fans (v0, vk, vk+1) of the polygons, in order"""
    off, pv = np.asarray(mesh["polygon_offsets"]), np.asarray(mesh["polygon_vertices"])
    tri, slot = [], []
    for f in range(len(off) - 1):
        v = pv[off[f]:off[f + 1]]
        for k in range(1, len(v) - 1):
            tri.append((v[0], v[k], v[k + 1]))
            slot.append(mesh["polygon_slot"][f])
    assert np.array_equal(np.asarray(mesh["triangles"]).reshape(-1, 3), np.array(tri, dtype=np.int64).reshape(-1, 3))
    assert np.array_equal(np.asarray(mesh["triangle_slot"]), np.array(slot, dtype=np.int64))

