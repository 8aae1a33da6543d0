"""ctypes loader of the HOST build of radfoam_amd/csrc/rf_locate.hpp (test harness; see locate_host.cpp): the passes of
radfoam.locate_tets / interpolate / interpolate_grad with a loop trip where the kernels have a lane.  Nothing raises here:
the walk hands the fault codes of rf_locate.hpp out as they are."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "..", "radfoam_amd", "csrc")
_SO = os.path.join(_HERE, "_build", "liblocate_host.so")
_SRC = [os.path.join(_HERE, "locate_host.cpp"), os.path.join(_CSRC, "rf_locate.hpp"), os.path.join(_CSRC, "rf_star.hpp")]


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
        _lib.locate_host_walk.restype = None
        _lib.locate_host_walk.argtypes = [P, U, P, P, U, U, P, P, U, U, P, P, P]
        _lib.locate_host_interpolate.restype = None
        _lib.locate_host_interpolate.argtypes = [P, U, P, U, U, P, U, U, P, P, U, P, P, P]
        _lib.locate_host_interpolate_grad.restype = None
        _lib.locate_host_interpolate_grad.argtypes = [P, U, P, U, U, P, U, U, P, P, U, P, P, P, P, P]
    return _lib


def _table(x):
    """a [T,4] table as 4-byte words (uint32 / int32 arrays) or int64"""
    x = np.asarray(x)
    return np.ascontiguousarray(x if x.dtype in (np.uint32, np.int32, np.int64) else x.astype(np.int64))


def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def walk(points, tets, adjacency, queries, start=None, max_hops=None) -> dict:
    """dict(tet int64[Q] with fault codes, hops int32[Q], predicates, exact) of the host build"""
    pts, q, rows, adj = _f32(points), _f32(queries).reshape(-1, 3), _table(tets), _table(adjacency)
    if rows.itemsize != adj.itemsize:
        rows, adj = rows.astype(np.int64), adj.astype(np.int64)
    nt, nq = len(rows), len(q)
    s = None if start is None else np.ascontiguousarray(np.asarray(start).astype(np.int64).reshape(-1))
    tet, hops, counters = np.zeros(nq, dtype=np.int64), np.zeros(nq, dtype=np.int32), np.zeros(2, dtype=np.int64)
    lib().locate_host_walk(pts.ctypes.data, len(pts), rows.ctypes.data, adj.ctypes.data, rows.itemsize, nt, q.ctypes.data,
                           None if s is None else s.ctypes.data, nq, min(nt, 2 ** 20) if max_hops is None else max_hops,
                           tet.ctypes.data, hops.ctypes.data, counters.ctypes.data)
    return dict(tet=tet, hops=hops, predicates=int(counters[0]), exact=int(counters[1]))


def _field(points, tets, values, queries, tet):
    pts, q, rows = _f32(points), _f32(queries).reshape(-1, 3), _table(tets)
    v = np.asarray(values)
    v = np.ascontiguousarray(v.reshape(len(pts), -1), dtype=np.float32 if v.dtype == np.float32 else np.float64)
    t = np.ascontiguousarray(np.asarray(tet).astype(np.int64).reshape(-1))
    return pts, rows, v, q, t


def interpolate(points, tets, values, queries, tet) -> dict:
    """dict(value f64[Q,C], weights f64[Q,4], gradient f64[Q,C,3]) of the host build; values float32 or float64"""
    pts, rows, v, q, t = _field(points, tets, values, queries, tet)
    nq, c = len(q), v.shape[1]
    value, weights, gradient = np.zeros((nq, c)), np.zeros((nq, 4)), np.zeros((nq, c, 3))
    lib().locate_host_interpolate(pts.ctypes.data, len(pts), rows.ctypes.data, rows.itemsize, len(rows), v.ctypes.data,
                                  v.itemsize, c, q.ctypes.data, t.ctypes.data, nq, value.ctypes.data, weights.ctypes.data,
                                  gradient.ctypes.data)
    return dict(value=value, weights=weights, gradient=gradient)


def interpolate_grad(points, tets, values, queries, tet, grad_value) -> dict:
    """dict(parts f64[Q,4,3+C], grad_points f64[N,3], grad_values f64[N,C], grad_queries f64[Q,3]) of the host build: the
    parts added per site in the kernel's order; C <= 8"""
    pts, rows, v, q, t = _field(points, tets, values, queries, tet)
    n, nq, c = len(pts), len(q), v.shape[1]
    assert c <= 8
    g = np.ascontiguousarray(np.asarray(grad_value, dtype=np.float64).reshape(nq, c))
    parts, gp, gv, gq = np.zeros((nq, 4, 3 + c)), np.zeros((n, 3)), np.zeros((n, c)), np.zeros((nq, 3))
    lib().locate_host_interpolate_grad(pts.ctypes.data, n, rows.ctypes.data, rows.itemsize, len(rows), v.ctypes.data,
                                       v.itemsize, c, q.ctypes.data, t.ctypes.data, nq, g.ctypes.data, parts.ctypes.data,
                                       gp.ctypes.data, gv.ctypes.data, gq.ctypes.data)
    return dict(parts=parts, grad_points=gp, grad_values=gv, grad_queries=gq)


def write_cases(path):
    """The plain arrays tests/host_harness/locate_sanitize.cpp reads: the 400-point cloud with the boundary queries (from
    row 0 and from the nearest site), the malformed tables and the capped walk, each with the fault kind its first faulted
    query must have (-1: none faults)."""
    from tests import locate_ref as R

    m, q = R.mesh("uniform", 400), R.queries("uniform", 400)["q"]
    rows, adj = m["tets"], m["tet_adjacency"]
    cases = [(rows, adj, None, q, len(rows), -1), (rows, adj, R.nearest_start(m, q), q, len(rows), -1),
             (rows, adj, None, q, 2, 4)]
    kinds = {"above": 0, "below": 0, "adjacency": 1, "flat": 2, "start": 3}
    cases += [(r, a, s, x, len(rows), kinds[name]) for name, (r, a, s, x) in R.malformed(m).items()]
    with open(path, "wb") as f:
        np.array([len(cases)], dtype=np.int64).tofile(f)
        for r, a, s, x, cap, kind in cases:
            np.array([len(m["points"]), len(r), len(x), s is not None, cap, kind], dtype=np.int64).tofile(f)
            _f32(m["points"]).tofile(f)
            np.ascontiguousarray(r, dtype=np.int64).tofile(f)
            np.ascontiguousarray(a, dtype=np.int64).tofile(f)
            _f32(x).tofile(f)
            if s is not None:
                np.ascontiguousarray(s, dtype=np.int64).tofile(f)
