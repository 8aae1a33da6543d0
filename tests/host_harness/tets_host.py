"""ctypes loader of the HOST build of radfoam_amd/csrc/rf_tets.hpp (test harness; see tets_host.cpp): the passes of
radfoam.delaunay_tets with a loop trip where the kernels have a lane."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from radfoam_amd.triangulation import TriangulationFailedError

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "..", "radfoam_amd", "csrc")
_SO = os.path.join(_HERE, "_build", "libtets_host.so")
_SRC = [os.path.join(_HERE, "tets_host.cpp"), os.path.join(_CSRC, "rf_tets.hpp"), os.path.join(_CSRC, "rf_star.hpp")]


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
        _lib.tets_host_build.restype = C.c_int
        _lib.tets_host_build.argtypes = [P, U, P, U, P, C.c_int, P]
        _lib.tets_host_fetch.restype = None
        _lib.tets_host_fetch.argtypes = [P, P, P, P, P]
    return _lib


def delaunay_tets(points, adjacency, offsets, tet_adjacency=True) -> dict:
    """dict(tets u32[T,4], vert_to_tet u32[N], tet_adjacency u32[T,4] or None, hull_faces, owned u32[N], code u8[N],
    big, huge) from the host build; RuntimeError / TriangulationFailedError as radfoam.delaunay_tets raises them"""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    adj = np.ascontiguousarray(np.asarray(adjacency).astype(np.int64).clip(-1, 2 ** 31 - 1).astype(np.int32))
    off = np.ascontiguousarray(np.asarray(offsets).astype(np.int64).clip(-1, 2 ** 31 - 1).astype(np.int32))
    n = pts.shape[0]
    assert pts.shape == (n, 3) and off.shape == (n + 1,)
    info = np.zeros(13, dtype=np.int64)
    rc = lib().tets_host_build(pts.ctypes.data, n, adj.ctypes.data, adj.shape[0], off.ctypes.data, int(tet_adjacency),
                               info.ctypes.data)
    if rc == 1:
        raise RuntimeError(f"row {info[2]} of the neighbour lists is malformed (code {info[3]})")
    if rc == 2:
        raise TriangulationFailedError(
            f"{info[4]} stars failed, {info[10]} star triangles for {info[0]} tetrahedra, {info[5]} sites with a flat or "
            f"repeated row, {info[6]} with an unmatched triangle, {info[7]} corners unconfirmed, {info[11]} faces seen more "
            f"than twice, {info[12]} unpaired faces for {info[1]} hull facets")
    nt = int(info[0])
    tets, v2t = np.zeros((nt, 4), dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    tadj = np.zeros((nt, 4), dtype=np.uint32) if tet_adjacency else None
    owned, code = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
    lib().tets_host_fetch(tets.ctypes.data, v2t.ctypes.data, None if tadj is None else tadj.ctypes.data, owned.ctypes.data,
                          code.ctypes.data)
    return dict(tets=tets, vert_to_tet=v2t, tet_adjacency=tadj, hull_faces=int(info[1]), owned=owned, code=code,
                big=int(info[8]), huge=int(info[9]))


def write_cases(path):
    """The plain arrays tests/host_harness/tets_sanitize.cpp reads: the 400-point cloud, the hub of 300 neighbours and the
    malformed (status 1) and stale (status 2) lists of the tests."""
    from tests import tets_ref as R

    ref, hub = R.cloud("uniform", 400), R.cloud("hub", 300)
    cases = [(ref["points"], ref["adjacency"], ref["offsets"], 0), (hub["points"], hub["adjacency"], hub["offsets"], 0)]
    cases += [(ref["points"], adj, off, 1) for adj, off in R.malformed_lists(ref).values()]
    cases += [(ref["points"], adj, off, 2) for adj, off in R.stale_lists(ref).values()]
    words = lambda x: np.asarray(x).astype(np.int64).clip(-1, 2 ** 31 - 1).astype(np.int32)
    with open(path, "wb") as f:
        np.array([len(cases)], dtype=np.uint32).tofile(f)
        for pts, adj, off, status in cases:
            np.array([len(pts), len(adj), status], dtype=np.uint32).tofile(f)
            np.ascontiguousarray(pts, dtype=np.float32).tofile(f)
            words(adj).tofile(f)
            words(off).tofile(f)
