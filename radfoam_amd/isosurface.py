"""The level set of a per-site value over the Delaunay tetrahedra as a welded, differentiable mesh (DESIGN.md,
"Isosurface of an interpolated field").

  isosurface                marching tetrahedra: the triangles of the level set over shared vertices; ``vertices``
                            carries autograd to ``points`` and ``values``
  isosurface_vertices       the vertices of a fixed topology again, each on its Delaunay edge
  isosurface_vertices_grad  its backward operator

The value interpolated linearly over every tetrahedron is a continuous field.  Its level set crosses a tetrahedron in a
triangle (one or three corners inside) or a quad (two), whose corners lie on edges between an inside and an outside site:
the corner on edge (a,b), a < b, is  p_a + t (p_b - p_a)  with  t = (level - v_a) / (v_b - v_a), and the pair (a,b) is
its key.  Every tetrahedron around the edge derives the same key, so equal keys are one vertex: welding needs no
tolerance on positions.  The kernels of csrc/rf_isosurface.hip behind the C-ABI of include/radfoam_hip_isosurface.h and
the torch restatement here share the definitions to the letter (csrc/rf_iso.hpp states them); the scan of the counts,
the welding (torch.unique over the packed keys) and the sort of the backward's gather are torch on the device on
either side.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _lib
from .scene_ops import _ptr, _stream
from .segments import _choose_backend


class IsoMesh(NamedTuple):
    vertices: torch.Tensor      # f64[V,3]; one row per crossed Delaunay edge
    vertex_sites: torch.Tensor  # int64[V,2]; (a, b) with a < b; rows in ascending lexicographic order
    vertex_t: torch.Tensor      # f64[V]; the interpolation parameter along a -> b, detached
    triangles: torch.Tensor     # int64[F,3]; indices into vertices; the normal points from value > level to the rest
    triangle_tet: torch.Tensor  # int64[F]; the tetrahedron of every triangle, ascending


def _parity(perm):
    return sum(perm[x] > perm[y] for x in range(4) for y in range(x + 1, 4)) % 2


def _case_tables():
    """(count int64[16], corners int64[16,2,3,2]): the triangles of every mask and the two row positions of each of
    their corners, from the case rule of DESIGN: (i,j,k,l) an even permutation of the row positions; i the lone corner
    and (j,k,l) the rest starting with the lowest (one or three inside), or i < j inside and (k,l) outside (two)."""
    count, corners = torch.zeros(16, dtype=torch.int64), torch.zeros((16, 2, 3, 2), dtype=torch.int64)
    for mask in range(1, 15):
        inside = [c for c in range(4) if mask >> c & 1]
        outside = [c for c in range(4) if not mask >> c & 1]
        if len(inside) == 2:
            i, j = inside
            k, l = outside if _parity([i, j] + outside) == 0 else outside[::-1]
            quad = [(i, k), (i, l), (j, l), (j, k)]
            tris = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
        else:
            lone, rest = (inside, outside) if len(inside) == 1 else (outside, inside)
            i, (j, k, l) = lone[0], rest
            if _parity([i, j, k, l]):
                k, l = l, k
            tris = [[(i, j), (i, k), (i, l)] if len(inside) == 1 else [(i, j), (i, l), (i, k)]]
        count[mask] = len(tris)
        corners[mask, :len(tris)] = torch.tensor(tris)
    return count, corners


_COUNT, _CORNERS = _case_tables()
_TABLES = {}


def _tables(dev):
    if dev not in _TABLES:
        _TABLES[dev] = (_COUNT.to(dev), _CORNERS.to(dev))
    return _TABLES[dev]


def _check_field(points, values):
    if points.dim() != 2 or points.size(-1) != 3 or not points.dtype.is_floating_point:
        raise RuntimeError("points must be a floating-point [N,3] tensor")
    if (not isinstance(values, torch.Tensor) or not values.dtype.is_floating_point or values.device != points.device
            or tuple(values.shape) != (points.size(0),)):
        raise RuntimeError(f"values must be a floating-point tensor of shape {[points.size(0)]} on the device of points")
    if points.size(0) >= 2 ** 31:
        raise RuntimeError("more than 2^31 points")


def _check_tets(points, tets):
    if (not isinstance(tets, torch.Tensor) or tets.dtype not in (torch.uint32, torch.int32, torch.int64) or tets.dim() != 2
            or tets.size(-1) != 4 or tets.device != points.device):
        raise RuntimeError("tets must be a uint32, int32 or int64 [T,4] tensor on the device of points")
    if tets.size(0) > 2 ** 30:
        raise RuntimeError("more than 2^30 tetrahedra")


def _check_sites(points, vertex_sites):
    if (not isinstance(vertex_sites, torch.Tensor) or vertex_sites.dtype != torch.int64 or vertex_sites.dim() != 2
            or vertex_sites.size(-1) != 2 or vertex_sites.device != points.device):
        raise RuntimeError("vertex_sites must be an int64 [V,2] tensor on the device of points")
    if vertex_sites.size(0) > 2 ** 30:
        raise RuntimeError("more than 2^30 vertices")


def _backend(points, values, backend):
    if backend is None and values.dtype != torch.float32:
        backend = "torch"
    chosen = _choose_backend(backend, points, "points")
    if chosen == "hip":
        _choose_backend("hip", values, "values")
    return chosen


def _range_error(tets, n):
    t64 = tets.to(torch.int64)
    first = int(torch.nonzero(((t64 < 0) | (t64 >= n)).any(1))[0])
    return RuntimeError(f"isosurface: tetrahedron {first} has a corner index outside [0, {n})")


# ---- the topology -----------------------------------------------------------------------------------------------------

def _extract_torch(p, tets, v, level):
    """(keys int64[F,3], triangle_tet int64[F]) or None: the three packed edge keys of every triangle in the final
    winding, tetrahedron after tetrahedron"""
    n, nt, dev = p.size(0), tets.size(0), p.device
    tets = tets.to(torch.int64)
    if bool(((tets < 0) | (tets >= n)).any()):
        raise _range_error(tets, n)
    count_of, corners_of = _tables(dev)
    tv = v.to(torch.float64)[tets]                                                   # [T,4]
    bits = torch.tensor([1, 2, 4, 8], dtype=torch.int64, device=dev)
    mask = ((tv > level).to(torch.int64) * bits).sum(1)
    mask = torch.where(torch.isfinite(tv).all(1), mask, torch.zeros_like(mask))
    counts = count_of[mask]
    triangle_tet = torch.repeat_interleave(torch.arange(nt, dtype=torch.int64, device=dev), counts)
    nf = triangle_tet.numel()
    if nf == 0:
        return None
    which = torch.arange(nf, dtype=torch.int64, device=dev) - (torch.cumsum(counts, 0) - counts)[triangle_tet]
    rows = tets[triangle_tet]                                                        # [F,4]
    q = p.to(torch.float64)[rows]                                                    # [F,4,3]
    d1, d2, d3 = q[:, 1] - q[:, 0], q[:, 2] - q[:, 0], q[:, 3] - q[:, 0]
    ax = d2[:, 1] * d3[:, 2] - d2[:, 2] * d3[:, 1]
    ay = d2[:, 2] * d3[:, 0] - d2[:, 0] * d3[:, 2]
    az = d2[:, 0] * d3[:, 1] - d2[:, 1] * d3[:, 0]
    det = (d1[:, 0] * ax + d1[:, 1] * ay) + d1[:, 2] * az
    corners = corners_of[mask[triangle_tet], which]                                  # [F,3,2]: row positions
    corners = torch.where((det < 0.0)[:, None, None], corners[:, [0, 2, 1]], corners)
    ends = rows.gather(1, corners.reshape(nf, 6)).reshape(nf, 3, 2)
    keys = ends.amin(2) * 2 ** 32 + ends.amax(2)
    return keys, triangle_tet


def _extract_hip(p, tets, v, level):
    n, nt, dev = p.size(0), tets.size(0), p.device
    lib = _lib.load()
    tets = tets.contiguous()
    if tets.data_ptr() % 16:
        tets = tets.clone()
    counts = torch.empty(nt, dtype=torch.uint8, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.rf_isosurface_count(_ptr(tets), tets.element_size(), nt, _ptr(v), n, level, _ptr(counts), _ptr(bad),
                                           _stream(dev)))
    ends = torch.cumsum(counts, 0, dtype=torch.int64)
    nf, flagged = torch.stack([ends[-1], bad[0].to(torch.int64)]).tolist()           # the one synchronisation
    if flagged:
        raise _range_error(tets, n)
    if nf == 0:
        return None
    keys = torch.empty((nf, 3), dtype=torch.int64, device=dev)
    triangle_tet = torch.empty(nf, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.rf_isosurface_emit(_ptr(tets), tets.element_size(), nt, _ptr(p), _ptr(v), n, level, _ptr(counts),
                                          _ptr(ends), nf, _ptr(keys), _ptr(triangle_tet), _stream(dev)))
    return keys, triangle_tet


# ---- the vertices of a fixed topology ---------------------------------------------------------------------------------

def _edges_torch(p, v, vertex_sites):
    """p_a, e = p_b - p_a, v_a, v_b in double and whether both sites are in range"""
    n, nv, dev = p.size(0), vertex_sites.size(0), p.device
    valid = ((vertex_sites >= 0) & (vertex_sites < n)).all(1)
    if n == 0:
        zero = torch.zeros((nv, 3), dtype=torch.float64, device=dev)
        return zero, zero, zero[:, 0], zero[:, 0], valid
    at = vertex_sites.clamp(0, n - 1)
    p64, v64 = p.to(torch.float64), v.to(torch.float64)
    pa = p64[at[:, 0]]
    return pa, p64[at[:, 1]] - pa, v64[at[:, 0]], v64[at[:, 1]], valid


def _point_torch(pa, e, va, vb, valid, level):
    """(x, t, D, ok) in the kernel's order of operations"""
    D = vb - va
    t = (level - va) / D
    x = pa + t[:, None] * e
    ok = valid & (D != 0.0) & torch.isfinite(t) & torch.isfinite(x).all(1)
    return x, t, D, ok


def _vertices_torch(p, v, vertex_sites, level):
    pa, e, va, vb, valid = _edges_torch(p, v, vertex_sites)
    x, t, _, ok = _point_torch(pa, e, va, vb, valid, level)
    nan = float("nan")
    return torch.where(ok[:, None], x, torch.full_like(x, nan)), torch.where(ok, t, torch.full_like(t, nan))


def _grad_parts_torch(p, v, vertex_sites, level, g):
    """f64[V,2,4]: (grad p, grad v) of a and of b for every vertex"""
    nv = vertex_sites.size(0)
    pa, e, va, vb, valid = _edges_torch(p, v, vertex_sites)
    _, t, D, ok = _point_torch(pa, e, va, vb, valid, level)
    dot = (g[:, 0] * e[:, 0] + g[:, 1] * e[:, 1]) + g[:, 2] * e[:, 2]
    ga = (dot * (level - vb)) / (D * D)
    gb = -((dot * (level - va)) / (D * D))
    parts = torch.stack([torch.cat([(1.0 - t)[:, None] * g, ga[:, None]], 1), torch.cat([t[:, None] * g, gb[:, None]], 1)], 1)
    ok = ok & torch.isfinite(parts).reshape(nv, 8).all(1)
    return torch.where(ok[:, None, None], parts, torch.zeros_like(parts))


def _vertices_grad_torch(p, v, vertex_sites, level, g):
    n = p.size(0)
    grad = torch.zeros((n, 4), dtype=torch.float64, device=p.device)
    if n and vertex_sites.size(0):
        parts = _grad_parts_torch(p, v, vertex_sites, level, g)
        grad.index_add_(0, vertex_sites.clamp(0, n - 1).reshape(-1), parts.reshape(-1, 4))
    return grad[:, :3].contiguous(), grad[:, 3].contiguous()


def _vertices_hip(p, v, vertex_sites, level):
    nv, dev = vertex_sites.size(0), p.device
    x = torch.empty((nv, 3), dtype=torch.float64, device=dev)
    t = torch.empty(nv, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().rf_isosurface_vertices(_ptr(p), _ptr(v), p.size(0), _ptr(vertex_sites), nv, level, _ptr(x),
                                                      _ptr(t), _stream(dev)))
    return x, t


def _vertices_grad_hip(p, v, vertex_sites, level, g):
    n, nv, dev = p.size(0), vertex_sites.size(0), p.device
    # the 2V incidences in order of site, ties in order of incidence: the order in which a site's lane adds them
    sites, order = torch.sort(vertex_sites.reshape(-1), stable=True)
    runs = torch.searchsorted(sites, torch.arange(n + 1, dtype=torch.int64, device=dev)).contiguous()
    parts = torch.empty((nv, 2, 4), dtype=torch.float64, device=dev)
    grad_points = torch.empty((n, 3), dtype=torch.float64, device=dev)
    grad_values = torch.empty(n, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().rf_isosurface_vertices_grad(_ptr(p), _ptr(v), n, _ptr(vertex_sites), nv, level, _ptr(g),
                                                           _ptr(order.contiguous()), _ptr(runs), _ptr(parts),
                                                           _ptr(grad_points), _ptr(grad_values), _stream(dev)))
    return grad_points, grad_values


def _grad_impl(backend, p, v, vertex_sites, level, g):
    if backend == "torch":
        return _vertices_grad_torch(p, v, vertex_sites, level, g)
    return _vertices_grad_hip(p, v, vertex_sites, level, g)


def _vertices_backend(points, values, vertex_sites, backend):
    _check_field(points, values)
    _check_sites(points, vertex_sites)
    return _backend(points, values, backend)


def isosurface_vertices_grad(points: torch.Tensor, values: torch.Tensor, vertex_sites: torch.Tensor, level: float,
                             grad_vertices: torch.Tensor, backend=None):
    """(f64[N,3], f64[N]): the gradients with respect to ``points`` and ``values`` of  sum_v grad_vertices[v] .
    vertices[v],  ``vertices`` being isosurface_vertices(points, values, vertex_sites, level).

    With g the upstream of the vertex on (a,b), D = v_b - v_a and e = p_b - p_a:  grad p_a = (1 - t) g,  grad p_b = t g,
    grad v_a = (g.e)(level - v_b) / D^2,  grad v_b = -(g.e)(level - v_a) / D^2, in double.  A vertex that is NaN in the
    forward or whose terms are not finite adds nothing.  The kernels write the two parts of every vertex once and one
    lane per site adds its own, in a fixed order: bit-reproducible, no atomics.  ``level`` is not differentiable.
    ``backend``: None (the kernels for float32 CUDA ``points`` and ``values``, torch otherwise), "hip" or "torch"."""
    chosen = _vertices_backend(points, values, vertex_sites, backend)
    nv = vertex_sites.size(0)
    if (not isinstance(grad_vertices, torch.Tensor) or grad_vertices.device != points.device
            or tuple(grad_vertices.shape) != (nv, 3) or not grad_vertices.dtype.is_floating_point):
        raise RuntimeError(f"grad_vertices must be a floating-point tensor of shape {[nv, 3]} on the device of points")
    return _grad_impl(chosen, points.detach().contiguous(), values.detach().contiguous(), vertex_sites.contiguous(),
                      float(level), grad_vertices.detach().to(torch.float64).contiguous())


class _IsoVertices(torch.autograd.Function):
    """(vertices, vertex_t) of fixed keys; vertex_t is not differentiable"""

    @staticmethod
    def forward(ctx, points, values, vertex_sites, level, backend):
        p, v = points.detach().contiguous(), values.detach().contiguous()
        ctx.save_for_backward(p, v, vertex_sites)
        ctx.level, ctx.backend, ctx.dtypes = level, backend, (points.dtype, values.dtype)
        x, t = (_vertices_torch if backend == "torch" else _vertices_hip)(p, v, vertex_sites, level)
        ctx.mark_non_differentiable(t)
        return x, t

    @staticmethod
    def backward(ctx, grad_vertices, _grad_t):
        p, v, vertex_sites = ctx.saved_tensors
        gp, gv = _grad_impl(ctx.backend, p, v, vertex_sites, ctx.level, grad_vertices.detach().to(torch.float64).contiguous())
        return gp.to(ctx.dtypes[0]), gv.to(ctx.dtypes[1]), None, None, None


def isosurface_vertices(points: torch.Tensor, values: torch.Tensor, vertex_sites: torch.Tensor, level: float,
                        backend=None) -> torch.Tensor:
    """f64[V,3]: for every row (a, b) of ``vertex_sites`` (int64[V,2]) the point  p_a + t (p_b - p_a),
    t = (level - v_a) / (v_b - v_a), in double and in this order of operations; differentiable in ``points`` and
    ``values`` (isosurface_vertices_grad, returned in their dtypes).  With the ``vertex_sites`` of an IsoMesh of the same
    inputs these are its ``vertices`` bit for bit, and they stay the vertices of that topology while the inputs move a
    little: nothing is extracted again.  On a topology gone stale t may leave [0,1] and the vertex extrapolates along its
    edge; a vertex with v_a == v_b, a site out of range or a result that is not finite is NaN and has no gradient.
    ``backend``: None (the kernels for float32 CUDA ``points`` and ``values``, torch otherwise), "hip" or "torch"."""
    chosen = _vertices_backend(points, values, vertex_sites, backend)
    return _IsoVertices.apply(points, values, vertex_sites.contiguous(), float(level), chosen)[0]


def _empty_mesh(dev):
    i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=dev)
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
    return IsoMesh(f64(0, 3), i64(0, 2), f64(0), i64(0, 3), i64(0))


def isosurface(points: torch.Tensor, tets: torch.Tensor, values: torch.Tensor, level: float, backend=None) -> IsoMesh:
    """Marching tetrahedra: the level set ``level`` of ``values`` (one per site, interpolated linearly over every
    tetrahedron of ``tets``, uint32, int32 or int64 [T,4], as Triangulation.tets() gives them) as a triangle mesh over
    shared vertices.

    A site is inside where its value is above ``level`` (strictly; NaN is outside); a tetrahedron with a value that is
    not finite emits nothing, one with one or three corners inside a triangle, one with two a quad as two triangles,
    in the order of ``tets``.  A vertex lies on a Delaunay edge (a,b), a < b, between an inside and an outside site; the
    pair is its key and equal keys are one vertex, so the mesh is welded without a tolerance.  Every triangle is wound
    with its normal from the inside to the outside, decided once per tetrahedron from the orientation of its four sites.
    With Delaunay tetrahedra of sites in general position and no inside site on the hull the mesh is closed and oriented
    (every directed edge once, its reverse once).  Exactly cospherical sites leave the tetrahedra to the triangulator
    and flat tetrahedra have an unreliable orientation: the result stays defined and deterministic there, closedness is
    not promised.

    ``vertices`` carries autograd to ``points`` and ``values`` (isosurface_vertices_grad, returned in their dtypes);
    ``vertex_t`` interpolates any per-site attribute to the vertices (torch.lerp(f[a], f[b], t)).  ``level`` is not
    differentiable.  Deterministic: two calls give the same bits.  Raises RuntimeError naming the first tetrahedron with
    a corner index outside [0, N); needs N < 2^31 and T <= 2^30.  No crossing: empty tensors.
    ``backend``: None (the kernels for float32 CUDA ``points`` and ``values``, torch otherwise), "hip" or "torch"."""
    _check_field(points, values)
    _check_tets(points, tets)
    chosen = _backend(points, values, backend)
    level = float(level)
    if tets.size(0) == 0:
        return _empty_mesh(points.device)
    p, v = points.detach().contiguous(), values.detach().contiguous()
    found = (_extract_torch if chosen == "torch" else _extract_hip)(p, tets, v, level)
    if found is None:
        return _empty_mesh(points.device)
    keys, triangle_tet = found
    uniq, inverse = torch.unique(keys.reshape(-1), return_inverse=True)              # ascending keys: ascending rows
    if uniq.numel() > 2 ** 30:
        raise RuntimeError("more than 2^30 vertices")
    vertex_sites = torch.stack([uniq >> 32, uniq & 0xFFFFFFFF], 1).contiguous()
    vertices, vertex_t = _IsoVertices.apply(points, values, vertex_sites, level, chosen)
    return IsoMesh(vertices, vertex_sites, vertex_t, inverse.reshape(-1, 3).contiguous(), triangle_tet)
