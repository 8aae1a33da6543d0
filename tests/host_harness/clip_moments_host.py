"""ctypes loader of the HOST build of radfoam_amd/csrc/rf_clip_moments.hpp (test harness; see clip_moments_host.cpp), and
the checks the CPU and GPU tests of the cell moments share."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from tests.host_harness import clip_host as H

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libclip_moments_host.so")
_CSRC = os.path.join(_HERE, "..", "..", "radfoam_amd", "csrc")
_SRC = [os.path.join(_HERE, "clip_moments_host.cpp"), os.path.join(_CSRC, "rf_clip_moments.hpp"),
        os.path.join(_CSRC, "rf_clip_grad.hpp"), os.path.join(_CSRC, "rf_clip.hpp")]

BAR = 1e-9      # |delta| <= BAR tr Q_exact[a] on each of the twelve numbers of cell a


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
        _lib.clip_moments_host_cell_moments.restype = C.c_int
        _lib.clip_moments_host_cell_moments.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                                        C.c_void_p, C.c_uint32] + [C.c_void_p] * 6
    return _lib


def cell_moments(points, adjacency, offsets, geo: dict, cap: int = 256) -> dict:
    """The host build of the serial cell over every cell: site f64[N,6], central f64[N,6], status u32[N] and ``bad``.
    ``geo`` is what clip_host.cell_geometry returned for the same cloud."""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    adj = np.ascontiguousarray(adjacency, dtype=np.uint32)
    off = np.ascontiguousarray(offsets, dtype=np.uint32)
    n, e = pts.shape[0], adj.shape[0]
    bbox = H.bbox_of(pts) if n else np.zeros(6, dtype=np.float32)
    vol = np.ascontiguousarray(geo["volume"], dtype=np.float64)
    cen = np.ascontiguousarray(geo["centroid"], dtype=np.float64)
    bnd = np.ascontiguousarray(geo["bounded"], dtype=np.uint8)
    assert vol.shape == (n,) and cen.shape == (n, 3) and bnd.shape == (n,)
    site, central, status = np.empty((n, 6)), np.empty((n, 6)), np.empty(n, dtype=np.uint32)
    bad = lib().clip_moments_host_cell_moments(pts.ctypes.data, n, adj.ctypes.data, off.ctypes.data, e, bbox.ctypes.data,
                                               cap, vol.ctypes.data, cen.ctypes.data, bnd.ctypes.data, site.ctypes.data,
                                               central.ctypes.data, status.ctypes.data)
    return dict(site=site, central=central, status=status, bad=bad)


# ---- what the CPU and GPU tests share ----------------------------------------------------------------------------------

_FORWARD = {}

# the cases compared with the exact reference and the cells the reference is restricted to (None: all of them; ring256's
# 256 ring cells would take the reference about 35 s)
EXACT_CASES = {"ring16": None, "ring17": None, "ring256": (0, 1), "hub64": None, "hub65": None, "hub200": None,
               "redo_spread": None, "clustered": None, "uniform400": None, "offset": None, "grid": None}


def host_forward(name: str, cap: int = 256) -> dict:
    """clip_host.cell_geometry of a case of clip_host.case, once"""
    if (name, cap) not in _FORWARD:
        c = H.case(name)
        _FORWARD[(name, cap)] = H.cell_geometry(c["points"], c["adjacency"], c["offsets"], cap=cap)
    return _FORWARD[(name, cap)]


def exact(name: str) -> dict:
    from tests import cell_moments_ref as M

    return M.exact_moments(H.case(name)["points"], cells=EXACT_CASES[name])


def check_against_exact(name: str, bounded, site, central, cells=None) -> float:
    """The bar of the cell moments: |delta| <= 1e-9 tr Q_exact[a] on each of the twelve numbers of every cell the exact
    reference calls bounded and the code called bounded (restricted to the cells the reference of the case works on, and
    to ``cells`` where given).  Every cell whose faces stay within R / 2 of their centres must be among them, every cell
    the code called unbounded (every open cell is one) is NaN in all twelve, every other finite.  Returns the worst ratio."""
    c, ref = H.case(name), exact(name)
    ex, R = c["exact"], c["R"]
    bounded = np.asarray(bounded, dtype=bool)
    assert site.shape == central.shape == (len(bounded), 6)
    assert np.array_equal(ref["open"], ex["open"])
    must = ~ex["open"] & (ex["extent"] < 0.5 * R)
    assert not bounded[ex["open"]].any() and bounded[must].all()
    assert np.isnan(site[~bounded]).all() and np.isnan(central[~bounded]).all()
    assert np.isfinite(site[bounded]).all() and np.isfinite(central[bounded]).all()
    if EXACT_CASES[name] is None:
        assert np.array_equal(ref["done"], ~ex["open"])
    cmp_ = ref["done"] & bounded          # holds every cell of ``must`` the reference worked on: none other is left out
    if cells is not None:
        pick = np.zeros_like(cmp_)
        pick[np.asarray(cells)] = True
        assert cmp_[pick].all()
        cmp_ = pick
    assert cmp_.any()
    unit = ref["trace_f"][cmp_][:, None]
    rs = (np.abs(site[cmp_] - ref["site_f"][cmp_]) / unit).max()
    rc = (np.abs(central[cmp_] - ref["central_f"][cmp_]) / unit).max()
    print(f"{name}: compared {cmp_.sum()} of {cmp_.size} cells ({must.sum()} must be bounded): worst |d site| / tr Q = "
          f"{rs:.3g}, |d central| / tr Q = {rc:.3g} (bar {BAR:.3g})")
    assert rs <= BAR and rc <= BAR
    return max(rs, rc)
