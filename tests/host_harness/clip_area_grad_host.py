"""ctypes loader of the HOST build of radfoam_amd/csrc/rf_clip_area_grad.hpp (test harness; see
clip_area_grad_host.cpp), and the checks the CPU and GPU tests of the face-area gradients share."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from tests.host_harness import clip_host as H

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libclip_area_grad_host.so")
_CSRC = os.path.join(_HERE, "..", "..", "radfoam_amd", "csrc")
_SRC = [os.path.join(_HERE, "clip_area_grad_host.cpp"), os.path.join(_CSRC, "rf_clip_area_grad.hpp"),
        os.path.join(_CSRC, "rf_clip.hpp")]
NO_LABEL = 0xFFFFFFFF


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
        _lib.clip_area_grad_host_face_area_grad.restype = C.c_int
        _lib.clip_area_grad_host_face_area_grad.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                                            C.c_void_p, C.c_uint32] + [C.c_void_p] * 5
        _lib.clip_area_grad_host_labelled_polygon.restype = C.c_int
        _lib.clip_area_grad_host_labelled_polygon.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                                              C.c_uint32, C.c_uint32] + [C.c_void_p] * 5
    return _lib


def _arrays(points, adjacency, offsets):
    pts = np.ascontiguousarray(points, dtype=np.float32)
    adj = np.ascontiguousarray(adjacency, dtype=np.uint32)
    off = np.ascontiguousarray(offsets, dtype=np.uint32)
    return pts, adj, off, (H.bbox_of(pts) if pts.shape[0] else np.zeros(6, dtype=np.float32))


def face_area_grad(points, adjacency, offsets, face_area, grad_face_area, cap: int = 256) -> dict:
    """The host build of the pre-pass and of the serial row over every cell: grad f64[N,3], weight f64[E] (the effective
    weight of every slot), status u32[N] and ``bad``.  ``face_area`` is what clip_host.cell_geometry returned."""
    pts, adj, off, bbox = _arrays(points, adjacency, offsets)
    n, e = pts.shape[0], adj.shape[0]
    area = np.ascontiguousarray(face_area, dtype=np.float64)
    g = np.ascontiguousarray(grad_face_area, dtype=np.float64)
    assert area.shape == (e,) and g.shape == (e,)
    grad, weight, status = np.empty((n, 3)), np.zeros(e), np.empty(n, dtype=np.uint32)
    bad = lib().clip_area_grad_host_face_area_grad(pts.ctypes.data, n, adj.ctypes.data, off.ctypes.data, e,
                                                   bbox.ctypes.data, cap, area.ctypes.data, g.ctypes.data,
                                                   weight.ctypes.data, grad.ctypes.data, status.ctypes.data)
    return dict(grad=grad, weight=weight, status=status, bad=bad)


def labelled_polygon(points, adjacency, offsets, a: int, slot: int, cap: int = 256):
    """dict(st f64[m,2], xyz f64[m,3] relative to p_a, label u32[m], plain f64[m',2]) of the face of adjacency slot
    ``slot`` of cell a: the labelled clipping and, in ``plain``, rf::clip::face_polygon's vertices; None past cap."""
    pts, adj, off, bbox = _arrays(points, adjacency, offsets)
    st, xyz, label, plain = np.empty((cap, 2)), np.empty((cap, 3)), np.empty(cap, dtype=np.uint32), np.empty((cap, 2))
    count = C.c_uint32(0)
    m = lib().clip_area_grad_host_labelled_polygon(pts.ctypes.data, adj.ctypes.data, off.ctypes.data, bbox.ctypes.data, a,
                                                   slot, cap, st.ctypes.data, xyz.ctypes.data, label.ctypes.data,
                                                   plain.ctypes.data, C.addressof(count))
    if m < 0:
        return None
    return dict(st=st[:m].copy(), xyz=xyz[:m].copy(), label=label[:m].copy(), plain=plain[:count.value].copy())


# ---- what the CPU and GPU tests share ----------------------------------------------------------------------------------

def unit_upstream(c: dict, geo: dict, seed: int = 0) -> np.ndarray:
    """g f64[E]: r / s with r uniform in [-1,1] and s the cube root of the smaller finite volume of the slot's two cells (1
    where both are unbounded), so that g A is of the order of the cell's size squared over its size; NaN on the slots of
    infinite area: nothing may read them.  Not symmetric: the two slots of a face draw their own r."""
    rng = np.random.default_rng(seed)
    rows, adj = c["rows"], c["adjacency"].astype(np.int64)
    v = np.minimum(geo["volume"][rows], geo["volume"][adj])
    size = np.cbrt(np.where(np.isfinite(v), v, 1.0))
    return np.where(np.isfinite(geo["face_area"]), rng.uniform(-1.0, 1.0, len(adj)) / size, np.nan)


def check_identities(points, face_area, g, grad, eps: float = 1e-9):
    """Translation sum_a grad p_a = 0, rotation sum_a p_a x grad p_a = 0 and scaling sum_a p_a . grad p_a = 2 sum g A over
    the finite slots (an area is homogeneous of degree 2), all to eps sum |p_a| |grad p_a| (the first times max |p|, to
    compare like with like)."""
    p = points.astype(np.float64)
    fin = np.isfinite(face_area)
    assert np.isfinite(grad).all()
    scale = (np.linalg.norm(p, axis=1) * np.linalg.norm(grad, axis=1)).sum()
    shift = np.abs(grad.sum(0)).max() * np.linalg.norm(p, axis=1).max()
    turn = np.abs(np.cross(p, grad).sum(0)).max()
    euler, want = (p * grad).sum(), 2.0 * (g[fin] * face_area[fin]).sum()
    print(f"identities: |sum grad| max|p| = {shift / scale:.3g}, |sum p x grad| = {turn / scale:.3g}, "
          f"|sum p.grad - 2 sum g A| = {abs(euler - want) / scale:.3g}, all of sum |p||grad| = {scale:.4g}")
    assert scale > 0.0 and shift <= eps * scale and turn <= eps * scale and abs(euler - want) <= eps * scale
