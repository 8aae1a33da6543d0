"""ctypes loader of the HOST build of radfoam_amd/csrc/rf_clip_grad.hpp (test harness; see clip_grad_host.cpp), and the
checks the CPU and GPU tests of the cell-geometry gradients share."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from tests.host_harness import clip_host as H

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libclip_grad_host.so")
_CSRC = os.path.join(_HERE, "..", "..", "radfoam_amd", "csrc")
_SRC = [os.path.join(_HERE, "clip_grad_host.cpp"), os.path.join(_CSRC, "rf_clip_grad.hpp"),
        os.path.join(_CSRC, "rf_clip.hpp")]


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
        _lib.clip_grad_host_cell_geometry_grad.restype = C.c_int
        _lib.clip_grad_host_cell_geometry_grad.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                                           C.c_void_p, C.c_uint32] + [C.c_void_p] * 7
        _lib.clip_grad_host_face_moments.restype = C.c_int
        _lib.clip_grad_host_face_moments.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                                     C.c_uint32, C.c_uint32, C.c_void_p]
    return _lib


def _f64(x, shape):
    if x is None:
        return None
    out = np.ascontiguousarray(x, dtype=np.float64)
    assert out.shape == shape
    return out


def cell_geometry_grad(points, adjacency, offsets, geo: dict, grad_volume, grad_centroid, cap: int = 256) -> dict:
    """The host build of the serial row over every cell: grad f64[N,3], status u32[N] and ``bad``.  ``geo`` is what
    clip_host.cell_geometry returned for the same cloud; either upstream may be None."""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    adj = np.ascontiguousarray(adjacency, dtype=np.uint32)
    off = np.ascontiguousarray(offsets, dtype=np.uint32)
    n, e = pts.shape[0], adj.shape[0]
    bbox = H.bbox_of(pts) if n else np.zeros(6, dtype=np.float32)
    vol, cen = _f64(geo["volume"], (n,)), _f64(geo["centroid"], (n, 3))
    bnd = np.ascontiguousarray(geo["bounded"], dtype=np.uint8)
    gv, gc = _f64(grad_volume, (n,)), _f64(grad_centroid, (n, 3))
    grad, status = np.empty((n, 3)), np.empty(n, dtype=np.uint32)
    ptr = lambda x: None if x is None else x.ctypes.data
    bad = lib().clip_grad_host_cell_geometry_grad(ptr(pts), n, ptr(adj), ptr(off), e, ptr(bbox), cap, ptr(vol), ptr(cen),
                                                  ptr(bnd), ptr(gv), ptr(gc), ptr(grad), ptr(status))
    return dict(grad=grad, status=status, bad=bad)


def face_moments(points, adjacency, offsets, a: int, slot: int, cap: int = 256):
    """(A, m f64[3], S f64[3,3]) of the face polygon of adjacency slot ``slot`` of cell a, in y = x - p_a"""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    adj = np.ascontiguousarray(adjacency, dtype=np.uint32)
    off = np.ascontiguousarray(offsets, dtype=np.uint32)
    bbox = H.bbox_of(pts)
    out = np.empty(10)
    m = lib().clip_grad_host_face_moments(pts.ctypes.data, adj.ctypes.data, off.ctypes.data, bbox.ctypes.data, a, slot,
                                          cap, out.ctypes.data)
    assert m >= 0
    S = np.empty((3, 3))
    S[np.triu_indices(3)] = out[4:]
    S = np.where(np.tri(3, dtype=bool), S.T, S)
    return out[0], out[1:4].copy(), S


# ---- what the CPU and GPU tests share ----------------------------------------------------------------------------------

_FORWARD = {}


def host_forward(key, c: dict) -> dict:
    """clip_host.cell_geometry of a case, once"""
    if key not in _FORWARD:
        _FORWARD[key] = H.cell_geometry(c["points"], c["adjacency"], c["offsets"])
        assert _FORWARD[key]["bad"] == 0
    return _FORWARD[key]


def unit_upstreams(geo: dict, seed: int = 0):
    """Unit upstreams per cell in units of the cell's own size s_a = V_a^(1/3): gV_a = r_a / s_a^2 and gC_a = r'_a with
    r, r' uniform in [-1,1], so that a cell's own terms of its row (gV A and (gC / V) S / l) are O(1).  On the unbounded
    cells they are NaN: nothing may read them."""
    rng = np.random.default_rng(seed)
    b = geo["bounded"]
    n = len(b)
    size = np.cbrt(np.where(b, geo["volume"], 1.0))
    gv = np.where(b, rng.uniform(-1.0, 1.0, n) / size ** 2, np.nan)
    gc = np.where(b[:, None], rng.uniform(-1.0, 1.0, (n, 3)), np.nan)
    return gv, gc


def check_identities(points, geo: dict, gv, gc, grad, eps: float = 1e-9):
    """Translation and scaling: sum_a grad p_a = sum gC_a (a translation moves no volume and every centroid with it: zero
    when only volumes are differentiated) and sum_a p_a . grad p_a = 3 sum gV_a V_a + sum gC_a . c_a (V is homogeneous
    of degree 3, c of degree 1), the right-hand sums over the bounded cells, both to eps sum |p_a| |grad p_a| (the first
    times max |p|, to compare like with like)."""
    p, b = points.astype(np.float64), geo["bounded"]
    assert np.isfinite(grad).all()
    scale = (np.linalg.norm(p, axis=1) * np.linalg.norm(grad, axis=1)).sum()
    shift = np.abs(grad.sum(0) - gc[b].sum(0)).max() * np.linalg.norm(p, axis=1).max()
    euler = (p * grad).sum()
    want = 3.0 * (gv[b] * geo["volume"][b]).sum() + (gc[b] * geo["centroid"][b]).sum()
    print(f"identities: |sum grad - sum gC| max|p| = {shift / scale:.3g}, |sum p.grad - (3 sum gV V + sum gC.c)| = "
          f"{abs(euler - want) / scale:.3g}, both of sum |p||grad| = {scale:.4g}")
    assert scale > 0.0 and shift <= eps * scale and abs(euler - want) <= eps * scale
