"""ctypes loader of the HOST build of radfoam_amd/csrc/rf_nearest.hpp (test harness; see nearest_host.cpp): the pass of
radfoam.locate_cells with a loop trip where the kernel has a lane.  Nothing raises here: the walk hands the fault codes of
rf_nearest.hpp out as they are."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "..", "radfoam_amd", "csrc")
_SO = os.path.join(_HERE, "_build", "libnearest_host.so")
_SRC = [os.path.join(_HERE, "nearest_host.cpp"), os.path.join(_CSRC, "rf_nearest.hpp"), os.path.join(_CSRC, "rf_star.hpp")]
MAX_SEEDS = 1024


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
        _lib.nearest_host_locate.restype = None
        _lib.nearest_host_locate.argtypes = [P, U, P, P, U, U, P, P, U, U, U, P, P, P]
        _lib.nearest_host_exact_closer.restype = C.c_int
        _lib.nearest_host_exact_closer.argtypes = [P]
    return _lib


def _list(x):
    """a list as 4-byte words (uint32 / int32 arrays) or int64"""
    x = np.asarray(x)
    return np.ascontiguousarray(x if x.dtype in (np.uint32, np.int32, np.int64) else x.astype(np.int64))


def locate(points, adj, offsets, queries, start=None, seeds=None, max_hops=None) -> dict:
    """dict(cell int64[Q] with fault codes, hops int32[Q], predicates, exact) of the host build; ``start``, ``seeds`` and
    ``max_hops`` as radfoam.locate_cells takes them"""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 3)
    a, o = _list(adj), _list(offsets)
    if a.itemsize != o.itemsize:
        a, o = a.astype(np.int64), o.astype(np.int64)
    n, nq = len(pts), len(q)
    s = None if start is None else np.ascontiguousarray(np.asarray(start).astype(np.int64).reshape(-1))
    num_seeds = 0 if s is not None else min(n, MAX_SEEDS if seeds is None else seeds)
    cell, hops, counters = np.zeros(nq, dtype=np.int64), np.zeros(nq, dtype=np.int32), np.zeros(2, dtype=np.int64)
    lib().nearest_host_locate(pts.ctypes.data, n, a.ctypes.data, o.ctypes.data, a.itemsize, len(a), q.ctypes.data,
                              None if s is None else s.ctypes.data, num_seeds, nq,
                              min(n, 2 ** 20) if max_hops is None else max_hops, cell.ctypes.data, hops.ctypes.data,
                              counters.ctypes.data)
    return dict(cell=cell, hops=hops, predicates=int(counters[0]), exact=int(counters[1]))


def exact_closer(pa, pb, q) -> int:
    p = np.ascontiguousarray(np.concatenate([pa, pb, q]), dtype=np.float32)
    return int(lib().nearest_host_exact_closer(p.ctypes.data))


def write_cases(path):
    """The plain arrays tests/host_harness/nearest_sanitize.cpp reads: the 400-point cloud with all query kinds (seeded,
    from site 0 and from given starts), the malformed tables and the capped walk, each with the fault kind its first
    faulted query must have (-1: none faults)."""
    from tests import nearest_ref as R

    m, q = R.cloud("uniform", 400), R.queries("uniform", 400)["q"]
    adj, off = m["adjacency"], m["offsets"]
    given = np.random.default_rng(3).integers(0, 400, len(q))
    cases = [(adj, off, None, q, 1024, 400, -1), (adj, off, None, q, 0, 400, -1), (adj, off, given, q, 0, 400, -1),
             (adj, off, None, q, 0, 2, 3)]
    kinds = {"start": 0, "offsets": 1, "past": 1, "above": 2, "below": 2}
    cases += [(a, o, s, x, 0, 400, kinds[name]) for name, (a, o, s, x) in R.malformed(m).items()]
    with open(path, "wb") as f:
        np.array([len(cases)], dtype=np.int64).tofile(f)
        for a, o, s, x, seeds, cap, kind in cases:
            np.array([len(m["points"]), len(a), len(x), s is not None, seeds, cap, kind], dtype=np.int64).tofile(f)
            np.ascontiguousarray(m["points"], dtype=np.float32).tofile(f)
            np.ascontiguousarray(a, dtype=np.int64).tofile(f)
            np.ascontiguousarray(o, dtype=np.int64).tofile(f)
            np.ascontiguousarray(x, dtype=np.float32).tofile(f)
            if s is not None:
                np.ascontiguousarray(s, dtype=np.int64).tofile(f)
