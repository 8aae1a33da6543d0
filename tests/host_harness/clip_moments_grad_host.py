"""ctypes loader of the HOST build of radfoam_amd/csrc/rf_clip_moments_grad.hpp (test harness; see
clip_moments_grad_host.cpp), and the checks the CPU and GPU tests of the cell-moment gradients share."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from tests.host_harness import clip_host as H

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libclip_moments_grad_host.so")
_CSRC = os.path.join(_HERE, "..", "..", "radfoam_amd", "csrc")
_SRC = [os.path.join(_HERE, "clip_moments_grad_host.cpp"), os.path.join(_CSRC, "rf_clip_moments_grad.hpp"),
        os.path.join(_CSRC, "rf_clip_moments.hpp"), os.path.join(_CSRC, "rf_clip_grad.hpp"),
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
        _lib.clip_moments_grad_host_cell_moments_grad.restype = C.c_int
        _lib.clip_moments_grad_host_cell_moments_grad.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                                                  C.c_uint32, C.c_void_p, C.c_uint32] + [C.c_void_p] * 7
        _lib.clip_moments_grad_host_moments3.restype = C.c_int
        _lib.clip_moments_grad_host_moments3.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_double, C.c_void_p]
    return _lib


def _f64(x, shape):
    if x is None:
        return None
    out = np.ascontiguousarray(x, dtype=np.float64)
    assert out.shape == shape
    return out


def cell_moments_grad(points, adjacency, offsets, geo: dict, grad_site_moment, grad_central_moment,
                      cap: int = 256) -> dict:
    """The host build of the serial row over every cell: grad f64[N,3], status u32[N] and ``bad``.  ``geo`` is what
    clip_host.cell_geometry returned for the same cloud; either upstream may be None."""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    adj = np.ascontiguousarray(adjacency, dtype=np.uint32)
    off = np.ascontiguousarray(offsets, dtype=np.uint32)
    n, e = pts.shape[0], adj.shape[0]
    bbox = H.bbox_of(pts) if n else np.zeros(6, dtype=np.float32)
    vol, cen = _f64(geo["volume"], (n,)), _f64(geo["centroid"], (n, 3))
    bnd = np.ascontiguousarray(geo["bounded"], dtype=np.uint8)
    gq, gc = _f64(grad_site_moment, (n, 6)), _f64(grad_central_moment, (n, 6))
    grad, status = np.empty((n, 3)), np.empty(n, dtype=np.uint32)
    ptr = lambda x: None if x is None else x.ctypes.data
    bad = lib().clip_moments_grad_host_cell_moments_grad(ptr(pts), n, ptr(adj), ptr(off), e, ptr(bbox), cap, ptr(vol),
                                                         ptr(cen), ptr(bnd), ptr(gq), ptr(gc), ptr(grad), ptr(status))
    return dict(grad=grad, status=status, bad=bad)


def moments3(s, t, R: float = 1e30):
    """rf::clip::moments3 of the polygon (s, t): f64[10] = a, s, t, ss, st, tt, sss, sst, stt, ttt about vertex 0"""
    s, t = np.ascontiguousarray(s, dtype=np.float64), np.ascontiguousarray(t, dtype=np.float64)
    assert s.shape == t.shape and s.ndim == 1
    out = np.empty(10)
    lib().clip_moments_grad_host_moments3(s.ctypes.data, t.ctypes.data, len(s), R, out.ctypes.data)
    return out


def write_arrays(name: str, path: str):
    """The rounded case ``name`` of tests/cell_geometry_grad_ref.case, its host forward and unit upstreams as the plain
    arrays clip_moments_grad_sanitize.cpp reads (the layout is described there)."""
    from tests import cell_geometry_grad_ref as G
    from tests.host_harness import clip_grad_host as HG

    c = G.case(name)
    geo = HG.host_forward(("rounded", name), c)
    gq, gc = unit_upstreams(geo)
    pts = np.ascontiguousarray(c["points"], dtype=np.float32)
    adj = np.ascontiguousarray(c["adjacency"], dtype=np.uint32)
    with open(path, "wb") as f:
        for x in (np.array([len(pts), len(adj)], dtype=np.uint32), pts, adj,
                  np.ascontiguousarray(c["offsets"], dtype=np.uint32), H.bbox_of(pts).astype(np.float32),
                  geo["volume"].astype(np.float64), geo["centroid"].astype(np.float64), geo["bounded"].astype(np.uint8),
                  gq, gc):
            f.write(np.ascontiguousarray(x).tobytes())


# ---- what the CPU and GPU tests share ----------------------------------------------------------------------------------

EPS = 1e-9
IDENTITY_CASES = ("uniform400", "offset", "clustered", "grid")
_FORWARD = {}


def host_forward(name: str) -> dict:
    """clip_host.cell_geometry and clip_moments_host.cell_moments of a case of clip_host.case, once"""
    from tests.host_harness import clip_moments_host as HM

    if name not in _FORWARD:
        c = H.case(name)
        geo = H.cell_geometry(c["points"], c["adjacency"], c["offsets"])
        mom = HM.cell_moments(c["points"], c["adjacency"], c["offsets"], geo)
        assert geo["bad"] == 0 and mom["bad"] == 0
        _FORWARD[name] = dict(geo, site=mom["site"], central=mom["central"])
    return _FORWARD[name]


def unit_upstreams(geo: dict, seed: int = 0):
    """(gQ, gC) f64[N,6]: r / s_a^4 with r uniform in [-1,1] and s_a = V_a^(1/3), so that a cell's own terms of its row
    are O(1).  On the unbounded cells they are NaN: nothing may read them."""
    rng = np.random.default_rng(seed)
    b = geo["bounded"]
    n = len(b)
    size = np.cbrt(np.where(b, geo["volume"], 1.0))[:, None]
    gq = np.where(b[:, None], rng.uniform(-1.0, 1.0, (n, 6)) / size ** 4, np.nan)
    gc = np.where(b[:, None], rng.uniform(-1.0, 1.0, (n, 6)) / size ** 4, np.nan)
    return gq, gc


def check_identities(points, fwd: dict, gq, gc, grad, eps: float = EPS):
    """Translation and scaling: sum_a grad p_a = 0 (both moments are relative: a translation changes neither) and
    sum_a p_a . grad p_a = 5 (sum <gQ, Q> + sum <gC, C>) (both are homogeneous of degree 5), the right-hand sums over the
    bounded cells, both to eps sum |p_a| |grad p_a| (the first times max |p|, to compare like with like, as
    clip_grad_host.check_identities does).  An absent upstream (None) counts as zero."""
    p, b = points.astype(np.float64), fwd["bounded"]
    assert np.isfinite(grad).all()
    scale = (np.linalg.norm(p, axis=1) * np.linalg.norm(grad, axis=1)).sum()
    shift = np.abs(grad.sum(0)).max() * np.linalg.norm(p, axis=1).max()
    euler = (p * grad).sum()
    want = 0.0
    if gq is not None:
        want += 5.0 * (gq[b] * fwd["site"][b]).sum()
    if gc is not None:
        want += 5.0 * (gc[b] * fwd["central"][b]).sum()
    print(f"identities: |sum grad| max|p| = {shift / scale:.3g}, |sum p.grad - 5 (sum <gQ,Q> + sum <gC,C>)| = "
          f"{abs(euler - want) / scale:.3g}, both of sum |p||grad| = {scale:.4g}")
    assert scale > 0.0 and shift <= eps * scale and abs(euler - want) <= eps * scale


def trace_upstream(geo: dict):
    """gQ of L = sum tr Q_a over the bounded cells (NaN elsewhere)"""
    return np.where(geo["bounded"][:, None], np.array([[1.0, 1.0, 1.0, 0.0, 0.0, 0.0]]), np.nan)


def check_closed_form(c: dict, geo: dict, grad, eps: float = EPS) -> int:
    """With gQ = (1,1,1,0,0,0) on every bounded cell and no central upstream, Psi_a = |x - p_a|^2 on both sides of a face
    between bounded cells, which vanishes on the bisector: grad p_a = 2 V_a (p_a - c_a) on every bounded cell all of whose
    neighbours are bounded, to eps V_a (longest |d_b| of the row) per component.  Returns how many were compared."""
    p, b = c["points"].astype(np.float64), geo["bounded"]
    off, adj = c["offsets"].astype(np.int64), c["adjacency"].astype(np.int64)
    count, worst = 0, 0.0
    for a in np.nonzero(b)[0]:
        nbrs = adj[off[a]:off[a + 1]]
        if not b[nbrs].all():
            continue
        want = 2.0 * geo["volume"][a] * (p[a] - geo["centroid"][a])
        unit = geo["volume"][a] * np.linalg.norm(p[nbrs] - p[a], axis=1).max()
        worst = max(worst, np.abs(grad[a] - want).max() / unit)
        count += 1
    print(f"closed form: {count} cells with bounded neighbours only, worst |grad - 2 V (p - c)| / (V max|d|) = {worst:.3g}")
    assert worst <= eps
    return count


def check_rows_against_host(name: str, device_grad, host_grad, seam, eps: float = EPS) -> float:
    """Device rows against the host build, which differ only in the order of the sum over a row's faces: eps of the row's
    scale per row.  With unit_upstreams a cell's own terms are O(1), and a neighbour much smaller than the cell adds
    terms of the order of their size ratio, so the scale of row a is max(1, max |host row a|).  Returns the worst ratio."""
    assert np.isfinite(device_grad).all() and np.isfinite(host_grad).all()
    scale = np.maximum(1.0, np.abs(host_grad).max(1))
    ratio = np.abs(device_grad - host_grad).max(1) / scale
    print(f"{name}: max |device - host| / scale = {ratio.max():.3g} over all rows, {ratio[seam].max():.3g} on the seam "
          f"rows (max |grad| = {np.abs(host_grad).max():.3g})")
    assert ratio.max() <= eps
    return float(ratio.max())
