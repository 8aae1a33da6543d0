"""The surface of selected Voronoi cells as a welded, differentiable mesh ("Welded surface mesh").

  cell_mesh           the faces between cells with ``inside`` set and their neighbours without, as polygons and triangles
                      over shared vertices; ``vertices`` carries autograd to ``points``
  mesh_vertices       the vertices of a fixed topology again, as circumcentres of their four sites
  mesh_vertices_grad  its backward operator

A corner of the polygon of face (a,b) lies where two further planes of a's row, of the neighbours c_in and c_out, meet
the face: it is the Voronoi vertex of the four sites, the circumcentre of a Delaunay tetrahedron, and the ascending
4-tuple of the sites is its key.  Every face around the vertex derives the same key from its own row, so equal keys are
one vertex: welding needs no tolerance on positions.  cell_mesh runs the kernels of csrc/rf_cell_mesh.hip behind the
C-ABI of include/radfoam_hip_mesh.h and has no CPU path; the welding itself (torch.unique over the packed keys) and the
sort of the backward's gather are torch on the device.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _lib
from .geometry import _STATUS_TEXT, _prepare, _run_geometry
from .scene_ops import _ptr, _stream
from .segments import _choose_backend

_FACE_STATUS_TEXT = dict(_STATUS_TEXT)
_FACE_STATUS_TEXT[3] = "the labelled clipping of a face gave another vertex count than cell_geometry"


class CellMesh(NamedTuple):
    vertices: torch.Tensor          # f64[V,3]; one row per distinct key
    vertex_sites: torch.Tensor      # int64[V,4]; the four sites, ascending in a row; rows in ascending lexicographic order
    polygon_offsets: torch.Tensor   # int64[F+1]
    polygon_vertices: torch.Tensor  # int64[C]; counter-clockwise seen from the outside cell
    polygon_slot: torch.Tensor      # int64[F]; the adjacency slot a -> b (inside[a], not inside[b]), ascending
    triangles: torch.Tensor         # int64[T,3]; the fan (v0, vk, vk+1) of every polygon
    triangle_slot: torch.Tensor     # int64[T]


def _check_sites(points, vertex_sites):
    if points.dim() != 2 or points.size(-1) != 3 or not points.dtype.is_floating_point:
        raise RuntimeError("points must be a floating-point [N,3] tensor")
    if (vertex_sites.dtype != torch.int64 or vertex_sites.dim() != 2 or vertex_sites.size(-1) != 4
            or vertex_sites.device != points.device):
        raise RuntimeError("vertex_sites must be an int64 [V,4] tensor on the device of points")
    if points.size(0) >= 2 ** 31 or vertex_sites.size(0) > 2 ** 30:
        raise RuntimeError("more than 2^31 points or 2^30 vertices")


def _edges_torch(points, vertex_sites):
    """p_0, d_1, d_2, d_3 in double and whether the key's four sites are all in range"""
    n = points.size(0)
    valid = ((vertex_sites >= 0) & (vertex_sites < n)).all(1)
    p = points.detach().to(torch.float64)[vertex_sites.clamp(0, max(n - 1, 0))] if n else \
        torch.zeros(vertex_sites.shape + (3,), dtype=torch.float64, device=points.device)
    p0 = p[:, 0]
    return p0, p[:, 1] - p0, p[:, 2] - p0, p[:, 3] - p0, valid


def _centre_torch(d1, d2, d3, valid):
    """(x, the three cross products, det, ok): x = M^-1 r by Cramer's rule, in the kernel's order of operations"""
    a, b, c = torch.linalg.cross(d2, d3), torch.linalg.cross(d3, d1), torch.linalg.cross(d1, d2)
    det = (d1[:, 0] * a[:, 0] + d1[:, 1] * a[:, 1]) + d1[:, 2] * a[:, 2]
    half_sq = lambda d: 0.5 * ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    r1, r2, r3 = half_sq(d1), half_sq(d2), half_sq(d3)
    x = ((r1[:, None] * a + r2[:, None] * b) + r3[:, None] * c) / det[:, None]
    ok = valid & (det != 0.0) & torch.isfinite(x).all(1)
    return x, (a, b, c), det, ok


def _mesh_vertices_torch(points, vertex_sites):
    p0, d1, d2, d3, valid = _edges_torch(points, vertex_sites)
    x, _, _, ok = _centre_torch(d1, d2, d3, valid)
    return torch.where(ok[:, None], p0 + x, torch.full_like(x, float("nan")))


def _mesh_vertices_grad_torch(points, vertex_sites, g):
    n, nv = points.size(0), vertex_sites.size(0)
    _, d1, d2, d3, valid = _edges_torch(points, vertex_sites)
    x, (a, b, c), det, ok = _centre_torch(d1, d2, d3, valid)
    dot = lambda u, w: (u[:, 0] * w[:, 0] + u[:, 1] * w[:, 1]) + u[:, 2] * w[:, 2]
    g1 = (dot(g, a) / det)[:, None] * (d1 - x)
    g2 = (dot(g, b) / det)[:, None] * (d2 - x)
    g3 = (dot(g, c) / det)[:, None] * (d3 - x)
    g0 = g - ((g1 + g2) + g3)
    parts = torch.stack([g0, g1, g2, g3], 1)                              # [V,4,3]
    ok = ok & torch.isfinite(parts).reshape(nv, 12).all(1)
    parts = torch.where(ok[:, None, None], parts, torch.zeros_like(parts))
    grad = torch.zeros((n, 3), dtype=torch.float64, device=points.device)
    if nv and n:
        grad.index_add_(0, vertex_sites.clamp(0, n - 1).reshape(-1), parts.reshape(-1, 3))
    return grad


def _mesh_vertices_hip(p, vertex_sites):
    nv, dev = vertex_sites.size(0), p.device
    out = torch.empty((nv, 3), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().rf_mesh_vertices(_ptr(p), p.size(0), _ptr(vertex_sites), nv, _ptr(out), _stream(dev)))
    return out


def _mesh_vertices_grad_hip(p, vertex_sites, g):
    n, nv, dev = p.size(0), vertex_sites.size(0), p.device
    # the 4V incidences in order of site, ties in order of incidence: the order in which a site's lane adds them
    sites, order = torch.sort(vertex_sites.reshape(-1), stable=True)
    runs = torch.searchsorted(sites, torch.arange(n + 1, dtype=torch.int64, device=dev)).contiguous()
    parts = torch.empty((nv, 4, 3), dtype=torch.float64, device=dev)
    grad = torch.empty((n, 3), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().rf_mesh_vertices_grad(_ptr(p), n, _ptr(vertex_sites), nv, _ptr(g), _ptr(order.contiguous()),
                                                     _ptr(runs), _ptr(parts), _ptr(grad), _stream(dev)))
    return grad


def _vertices_backend(points, vertex_sites, backend):
    _check_sites(points, vertex_sites)
    return _choose_backend(backend, points, "points")


def _grad_impl(backend, p, vertex_sites, g):
    if backend == "torch":
        return _mesh_vertices_grad_torch(p, vertex_sites, g)
    return _mesh_vertices_grad_hip(p, vertex_sites, g)


def mesh_vertices_grad(points: torch.Tensor, vertex_sites: torch.Tensor, grad_vertices: torch.Tensor,
                       backend=None) -> torch.Tensor:
    """f64[N,3]: the gradient with respect to ``points`` of  sum_v grad_vertices[v] . vertices[v],  ``vertices`` being
    mesh_vertices(points, vertex_sites).

    With d_i = p_i - p_0 over a key's sites, M the matrix of rows d_i, x = M^-1 (|d_i|^2 / 2) and y = M^-T g:
    grad p_i = y_i (d_i - x) for i = 1..3 and grad p_0 = g - their sum, in double.  A vertex that is NaN in the forward
    (exactly coplanar sites, a site out of range) or whose terms are not finite adds nothing.  The kernels write the four
    vectors of every vertex once and one lane per site adds its own, in a fixed order: bit-reproducible, no atomics.
    ``backend``: None (the kernels for float32 CUDA ``points``, torch otherwise), "hip" or "torch"."""
    chosen = _vertices_backend(points, vertex_sites, backend)
    nv = vertex_sites.size(0)
    if (not isinstance(grad_vertices, torch.Tensor) or grad_vertices.device != points.device
            or tuple(grad_vertices.shape) != (nv, 3) or not grad_vertices.dtype.is_floating_point):
        raise RuntimeError(f"grad_vertices must be a floating-point tensor of shape {[nv, 3]} on the device of points")
    return _grad_impl(chosen, points.detach().contiguous(), vertex_sites.contiguous(),
                      grad_vertices.detach().to(torch.float64).contiguous())


class _MeshVertices(torch.autograd.Function):
    """the vertices of fixed keys: evaluated as circumcentres, or (``stored``) picked from the clipped corners"""

    @staticmethod
    def forward(ctx, points, vertex_sites, backend, stored, first):
        p = points.detach().contiguous()
        ctx.save_for_backward(p, vertex_sites)
        ctx.backend, ctx.points_dtype = backend, points.dtype
        if stored is not None:
            return stored[first]
        return _mesh_vertices_torch(p, vertex_sites) if backend == "torch" else _mesh_vertices_hip(p, vertex_sites)

    @staticmethod
    def backward(ctx, grad_vertices):
        p, vertex_sites = ctx.saved_tensors
        grad = _grad_impl(ctx.backend, p, vertex_sites, grad_vertices.detach().to(torch.float64).contiguous())
        return grad.to(ctx.points_dtype), None, None, None, None


def mesh_vertices(points: torch.Tensor, vertex_sites: torch.Tensor, backend=None) -> torch.Tensor:
    """f64[V,3]: the circumcentre of the four rows of ``points`` every row of ``vertex_sites`` (int64[V,4]) names,
    computed in double relative to the row's first site; differentiable in ``points`` (mesh_vertices_grad, returned in the
    dtype of ``points``).  With the ``vertex_sites`` of a CellMesh these are its ``vertices`` to rounding, and they stay the
    vertices of that topology while the sites move a little: no clipping is run.  NaN where a site is out of range, the
    four sites are exactly coplanar or the result is not finite; nearly coplanar sites give large finite values.
    ``backend``: None (the kernels for float32 CUDA ``points``, torch otherwise), "hip" or "torch"."""
    chosen = _vertices_backend(points, vertex_sites, backend)
    return _MeshVertices.apply(points, vertex_sites.contiguous(), chosen, None, None)


def _empty_mesh(dev):
    i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=dev)
    return CellMesh(torch.zeros((0, 3), dtype=torch.float64, device=dev), i64(0, 4), i64(1), i64(0), i64(0), i64(0, 3),
                    i64(0))


def _emit(p, adj, off, bbox, face_vertices, inside):
    """(slots int64[F], polygon_offsets int64[F+1], corner_xyz f64[C,3], corner_sites int64[C,4]); one synchronisation
    for the sizes and one to read whether a face was refused"""
    n, e, dev = p.size(0), adj.numel(), p.device
    lib = _lib.load()
    mask = inside.contiguous().view(torch.uint8)
    counts = torch.zeros(e, dtype=torch.int32, device=dev)         # vertices - 2 of every straddling face, as cell_surface
    with torch.cuda.device(dev):
        _lib.check(lib.rf_cell_surface_count(n, _ptr(adj), _ptr(off), e, _ptr(mask), _ptr(face_vertices), _ptr(counts),
                                             _stream(dev)))
    slots = torch.nonzero(counts).reshape(-1)                      # ascending adjacency slots
    nf = slots.numel()
    offsets = torch.zeros(nf + 1, dtype=torch.int64, device=dev)
    if nf:
        torch.cumsum(face_vertices[slots].to(torch.int64), 0, out=offsets[1:])
    nc = int(offsets[-1])
    if nf >= 2 ** 32 or nc >= 2 ** 62:
        raise RuntimeError("more than 2^32 faces")
    xyz = torch.empty((nc, 3), dtype=torch.float64, device=dev)
    sites = torch.empty((nc, 4), dtype=torch.int32, device=dev)
    status = torch.empty(nf, dtype=torch.uint8, device=dev)
    ws = torch.empty(max(int(lib.rf_cell_mesh_emit_workspace_bytes(nf)), 256), dtype=torch.uint8, device=dev)
    begins = offsets[:-1].contiguous()
    with torch.cuda.device(dev):
        _lib.check(lib.rf_cell_mesh_emit(_ptr(p), n, _ptr(adj), _ptr(off), e, _ptr(bbox), _ptr(face_vertices), _ptr(slots),
                                         _ptr(begins), nf, nc, _ptr(xyz), _ptr(sites), _ptr(status), _ptr(ws), ws.numel(),
                                         _stream(dev)))
    if nf:
        worst, face = status.max(0)
        worst, slot = torch.stack([worst.to(torch.int64), slots[face]]).tolist()
        if worst:
            cell = int(torch.searchsorted(off.to(torch.int64) & 0xFFFFFFFF, slot, right=True)) - 1
            raise RuntimeError(f"cell_mesh: cell {cell} is not supported: {_FACE_STATUS_TEXT.get(worst, worst)}")
    return slots, offsets, xyz, sites.to(torch.int64)


def _weld(corner_sites):
    """(vertex_sites int64[V,4] in ascending lexicographic order, the vertex of every corner int64[C], the lowest corner
    of every vertex int64[V]).  The keys are packed into two signed words (sites below 2^31), so the order of the words
    is the order of the rows."""
    nc, dev = corner_sites.size(0), corner_sites.device
    words = torch.stack([corner_sites[:, 0] * 2 ** 32 + corner_sites[:, 1], corner_sites[:, 2] * 2 ** 32 + corner_sites[:, 3]], 1)
    uniq, inverse = torch.unique(words, dim=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    first = torch.full((uniq.size(0),), nc, dtype=torch.int64, device=dev)
    first.scatter_reduce_(0, inverse, torch.arange(nc, dtype=torch.int64, device=dev), "amin")   # a minimum: any order
    return corner_sites[first].contiguous(), inverse, first


def _fans(offsets, polygon_vertices, slots):
    """triangles int64[T,3] and their slots: (v0, vk, vk+1), k = 1 .. m - 2, polygon after polygon"""
    dev = offsets.device
    per = offsets[1:] - offsets[:-1] - 2
    poly = torch.repeat_interleave(torch.arange(per.numel(), device=dev), per)
    ends = torch.cumsum(per, 0)
    k = torch.arange(poly.numel(), device=dev) - (ends - per)[poly] + 1
    base = offsets[:-1][poly]
    tri = torch.stack([polygon_vertices[base], polygon_vertices[base + k], polygon_vertices[base + k + 1]], 1)
    return tri.contiguous(), slots[poly].contiguous()


def cell_mesh(points: torch.Tensor, point_adjacency: torch.Tensor, point_adjacency_offsets: torch.Tensor,
              inside: torch.Tensor) -> CellMesh:
    """The surface cell_surface extracts -- every face between a cell with ``inside`` set and a neighbour without --
    as a mesh over shared vertices.

    One polygon per straddling adjacency slot a -> b of three or more vertices, in slot order, wound counter-clockwise
    seen from the outside cell b (cell_surface's winding); ``triangles`` are the polygons' fans, cell_surface's triangles
    in its order, and ``triangle_slot`` its ``edge``.  A corner's key is the ascending 4-tuple of a, b and the two
    neighbours whose planes meet at it; corners of equal keys are one vertex, positioned by the lowest-numbered corner that
    carries the key: ``vertices[triangles]`` equals cell_surface's triangles bit for bit where that corner is the
    triangle's own and to rounding elsewhere.  On sites in general position the mesh is closed and oriented (every
    directed edge once, its reverse once).  Where more than four sites are cospherical (an unjittered grid) rounding
    decides which of two coincident planes labels an edge, so coincident vertices may keep different keys and stay
    unwelded: the geometry is still cell_surface's, no closedness is promised, and there is no welding by position.

    With ``points.requires_grad``, ``vertices`` carries autograd: the values are the clipped ones, the backward is
    mesh_vertices_grad (each vertex as the circumcentre of its key's sites), returned in the dtype of ``points``.

    Deterministic: two calls give the same bits.  Raises ValueError if ``inside`` selects an unbounded cell and
    RuntimeError naming the cell like cell_geometry; needs fewer than 2^31 points.  No selected cell: empty tensors."""
    p, adj, off, bbox = _prepare(points, point_adjacency, point_adjacency_offsets)
    n, dev = p.size(0), p.device
    if not inside.is_cuda or inside.device != dev or inside.dtype != torch.bool or inside.shape != (n,):
        raise RuntimeError("inside must be a bool[N] CUDA tensor on the device of points")
    if n >= 2 ** 31:
        raise RuntimeError("cell_mesh takes fewer than 2^31 points")
    if n == 0 or not bool(inside.any()):
        return _empty_mesh(dev)
    geo, face_vertices = _run_geometry(p, adj, off, bbox)
    if bool((inside & ~geo.bounded).any()):
        raise ValueError("cell_mesh: inside selects an unbounded cell")
    slots, offsets, corner_xyz, corner_sites = _emit(p, adj, off, bbox, face_vertices, inside)
    if slots.numel() == 0:
        return _empty_mesh(dev)
    vertex_sites, polygon_vertices, first = _weld(corner_sites)
    if points.requires_grad and torch.is_grad_enabled():
        vertices = _MeshVertices.apply(points, vertex_sites, "hip", corner_xyz, first)
    else:
        vertices = corner_xyz[first]
    triangles, triangle_slot = _fans(offsets, polygon_vertices, slots)
    return CellMesh(vertices, vertex_sites, offsets, polygon_vertices, slots, triangles, triangle_slot)
