"""Voronoi cell geometry on the device: what a cell of the foam IS ("Cell geometry").

  cell_geometry   volume, centroid, boundedness of every cell and the area of every face, in double
  cell_surface    the faces between selected and unselected cells, as triangles: the foam's own watertight surface of
                  e.g. ``density > tau``
  cell_geometry_grad            the gradient of a function of the volumes and centroids with respect to ``points``
  face_area_grad                the gradient of a function of the face areas with respect to ``points``
  differentiable_cell_geometry  cell_geometry whose volume and centroid (and, on request, face areas) carry autograd to
                                ``points``
  cell_geometry_in_box          cell_geometry of the cells clipped to an axis-aligned box: every cell bounded, plus the
                                area each cell takes of each wall
  cell_geometry_in_box_grad     the gradient of a function of the boxed volumes and centroids with respect to ``points``
  face_area_in_box_grad         the gradient of a function of the boxed face and wall areas with respect to ``points``
  differentiable_cell_geometry_in_box  cell_geometry_in_box whose volume and centroid (and, on request, face and wall
                                areas) carry autograd to ``points``
  cell_moments    the second moment of every cell about its site and about its centroid: the cell's shape
  cell_moments_grad             the gradient of a function of the second moments with respect to ``points``
  differentiable_cell_moments   cell_moments whose moments, volume and centroid carry autograd to ``points``
  cell_moments_in_box           cell_moments of the cells clipped to an axis-aligned box: every cell, hull cells and sites
                                outside the box included, has its second moments
  cell_moments_in_box_grad      the gradient of a function of the boxed second moments, volumes and centroids with respect
                                to ``points``, in one launch
  differentiable_cell_moments_in_box  cell_moments_in_box whose moments, volume and centroid carry autograd to ``points``

Cell ``a`` is the intersection of the half-spaces of its row of ``point_adjacency`` (taken as given); no tetrahedra are
involved.  All take CUDA (HIP) tensors and run the kernels of csrc/rf_cell_geometry.hip, csrc/rf_cell_geometry_grad.hip,
csrc/rf_face_area_grad.hip, csrc/rf_cell_moments.hip, csrc/rf_cell_moments_grad.hip, csrc/rf_cell_box.hip,
csrc/rf_cell_box_grad.hip, csrc/rf_cell_box_moments.hip, csrc/rf_cell_box_moments_grad.hip and
csrc/rf_cell_box_area_grad.hip behind the C-ABI of
include/radfoam_hip_geometry.h,
include/radfoam_hip_geometry_grad.h, include/radfoam_hip_face_area_grad.h, include/radfoam_hip_moments.h,
include/radfoam_hip_moments_grad.h, include/radfoam_hip_box.h, include/radfoam_hip_box_grad.h,
include/radfoam_hip_box_moments.h, include/radfoam_hip_box_moments_grad.h and include/radfoam_hip_box_area_grad.h; there
is no CPU path.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import torch

from . import _lib
from .scene_ops import _check_f32_cuda, _ptr, _stream

_STATUS_TEXT = {1: "a face outgrew 256 vertices while it was clipped",
                2: "its adjacency row is malformed (offsets out of order, an index out of range, the site itself or "
                   "a duplicate of it)"}


class CellGeometry(NamedTuple):
    volume: torch.Tensor      # f64[N]; +inf for an unbounded cell
    centroid: torch.Tensor    # f64[N,3]; NaN for an unbounded cell
    bounded: torch.Tensor     # bool[N]
    face_area: torch.Tensor   # f64[E], aligned with point_adjacency; +inf for an unbounded face


class BoxedCellGeometry(NamedTuple):
    volume: torch.Tensor      # f64[N]; finite, >= 0 up to rounding
    centroid: torch.Tensor    # f64[N,3]; NaN for an empty cell
    nonempty: torch.Tensor    # bool[N]: volume > 0
    face_area: torch.Tensor   # f64[E], aligned with point_adjacency: the part of the face inside the box; finite
    wall_area: torch.Tensor   # f64[N,6]: the part of each wall that bounds the cell, walls x-, x+, y-, y+, z-, z+


class CellMoments(NamedTuple):
    site_moment: torch.Tensor      # f64[N,6]: int (x - p)(x - p)^T dx as xx, yy, zz, xy, xz, yz; NaN for an unbounded cell
    central_moment: torch.Tensor   # f64[N,6]: the same about the centroid; NaN for an unbounded cell
    geometry: CellGeometry         # the volumes and centroids the central moment was formed with


class BoxedCellMoments(NamedTuple):
    site_moment: torch.Tensor      # f64[N,6]: int over cell n box of (x - p)(x - p)^T dx as xx, yy, zz, xy, xz, yz; finite
    central_moment: torch.Tensor   # f64[N,6]: the same about the centroid; NaN for an empty cell
    geometry: BoxedCellGeometry    # the volumes and centroids the central moment was formed with


def _index_tensor(name, t, device):
    """uint32 / int32 / int64 -> the uint32 words the kernels read (as a contiguous int32-typed tensor)."""
    if not t.is_cuda or t.device != device:
        raise RuntimeError(f"{name} must be a CUDA tensor on the device of points")
    if t.dtype == torch.uint32:
        return t.contiguous().view(torch.int32)
    if t.dtype == torch.int32:
        return t.contiguous()
    if t.dtype == torch.int64:
        return t.to(torch.int32).contiguous()     # values below 2^32 keep their low word
    raise RuntimeError("point_adjacency and point_adjacency_offsets must have uint32, int32 or int64 dtype")


def _prepare(points, point_adjacency, point_adjacency_offsets):
    _check_f32_cuda("points", points)
    if points.dim() != 2 or points.size(-1) != 3:
        raise RuntimeError("points must be [N,3]")
    p = points.detach().contiguous()
    adj = _index_tensor("point_adjacency", point_adjacency, p.device)
    off = _index_tensor("point_adjacency_offsets", point_adjacency_offsets, p.device)
    if adj.dim() != 1 or off.dim() != 1 or off.numel() != p.size(0) + 1:
        raise RuntimeError("expected point_adjacency [E] and point_adjacency_offsets [N+1]")
    if p.size(0) >= 2 ** 32 - 1 or adj.numel() >= 2 ** 32:
        raise RuntimeError("more than 2^32 points or adjacency entries")
    bbox = (torch.cat([p.min(0).values, p.max(0).values]) if p.size(0)
            else torch.zeros(6, dtype=torch.float32, device=p.device))
    return p, adj, off, bbox


def _opt(t):
    return None if t is None else _ptr(t)


def _run_cells(name, entry, p, adj, off, bbox, *tensors, six=(), edge_workspace=False):
    """Calls ``rf_<entry>`` of the library: (points, N, adjacency, offsets, E, bbox, *six, *tensors, status, workspace,
    bytes, stream), a tensor that is None going as a null pointer.  One synchronisation, to read whether a cell was
    refused; then RuntimeError "<name>: cell <i> is not supported: ..."."""
    n, e, dev = p.size(0), adj.numel(), p.device
    lib = _lib.load()
    status = torch.empty(n, dtype=torch.uint8, device=dev)
    size = getattr(lib, f"rf_{entry}_workspace_bytes")
    ws = torch.empty(max(int(size(n, e) if edge_workspace else size(n)), 256), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = getattr(lib, f"rf_{entry}")(_ptr(p), n, _ptr(adj), _ptr(off), e, _ptr(bbox), *six, *map(_opt, tensors),
                                         _ptr(status), _ptr(ws), ws.numel(), _stream(dev))
    _lib.check(rc)
    if n:
        worst, cell = status.max(0)
        worst, cell = torch.stack([worst.to(torch.int64), cell]).tolist()      # the one synchronisation
        if worst:
            raise RuntimeError(f"{name}: cell {cell} is not supported: {_STATUS_TEXT.get(worst, worst)}")


def _run_geometry(p, adj, off, bbox):
    """(CellGeometry, face_vertices int32[E]); one synchronisation, to read whether a cell was refused."""
    n, e, dev = p.size(0), adj.numel(), p.device
    volume = torch.empty(n, dtype=torch.float64, device=dev)
    centroid = torch.empty((n, 3), dtype=torch.float64, device=dev)
    bounded = torch.empty(n, dtype=torch.uint8, device=dev)
    face_area = torch.empty(e, dtype=torch.float64, device=dev)
    face_vertices = torch.empty(e, dtype=torch.int32, device=dev)
    _run_cells("cell_geometry", "cell_geometry", p, adj, off, bbox, volume, centroid, bounded, face_area, face_vertices)
    return CellGeometry(volume, centroid, bounded.bool(), face_area), face_vertices


def cell_geometry(points: torch.Tensor, point_adjacency: torch.Tensor,
                  point_adjacency_offsets: torch.Tensor) -> CellGeometry:
    """Volume f64[N], centroid f64[N,3], bounded bool[N] of every Voronoi cell and face_area f64[E] of every face
    (aligned with ``point_adjacency``), computed in double from the fp32 points.

    A face is the bisector plane of (a,b) clipped by the other half-spaces of a's row, starting from a square of
    half-side 4 * |bbox diagonal|; it is unbounded (area +inf) when a piece of that square survives.  A cell with an
    unbounded face, or with no neighbours, is unbounded: volume +inf, centroid NaN, bounded False; its bounded faces
    keep their finite areas.  Index tensors may be uint32, int32 or int64.  Raises RuntimeError naming the cell if a
    face needs more than 256 vertices or a row is malformed."""
    return _run_geometry(*_prepare(points, point_adjacency, point_adjacency_offsets))[0]


def _box_six(box):
    """``box`` as six Python floats (lo, hi): a sequence or tensor of six numbers, or a [2,3] tensor; ValueError unless
    they are finite with lo < hi in every axis."""
    try:
        flat = box.detach().reshape(-1).tolist() if isinstance(box, torch.Tensor) else [x for x in box]
        if len(flat) == 2 and not isinstance(box, torch.Tensor):       # ((lo), (hi))
            flat = [x for part in flat for x in part]
        six = [float(x) for x in flat]
    except (TypeError, ValueError) as exc:
        raise ValueError("box must be six numbers (lo[3], hi[3])") from exc
    if len(six) != 6:
        raise ValueError(f"box must be six numbers (lo[3], hi[3]), not {len(six)}")
    if not all(math.isfinite(x) for x in six) or not all(math.isfinite(six[k + 3] - six[k]) for k in range(3)):
        raise ValueError("box must be finite")
    if not all(six[k] < six[k + 3] for k in range(3)):
        raise ValueError("box must have lo < hi in every axis")
    return six


def _run_geometry_in_box(p, adj, off, bbox, six):
    """(BoxedCellGeometry, face_vertices int32[E], wall_vertices int32[N,6]); one synchronisation, to read whether a cell
    was refused."""
    n, e, dev = p.size(0), adj.numel(), p.device
    volume = torch.empty(n, dtype=torch.float64, device=dev)
    centroid = torch.empty((n, 3), dtype=torch.float64, device=dev)
    nonempty = torch.empty(n, dtype=torch.uint8, device=dev)
    face_area = torch.empty(e, dtype=torch.float64, device=dev)
    face_vertices = torch.empty(e, dtype=torch.int32, device=dev)
    wall_area = torch.empty((n, 6), dtype=torch.float64, device=dev)
    wall_vertices = torch.empty((n, 6), dtype=torch.int32, device=dev)
    _run_cells("cell_geometry_in_box", "cell_box", p, adj, off, bbox, volume, centroid, nonempty, face_area,
               face_vertices, wall_area, wall_vertices, six=six)
    return BoxedCellGeometry(volume, centroid, nonempty.bool(), face_area, wall_area), face_vertices, wall_vertices


def cell_geometry_in_box(points: torch.Tensor, point_adjacency: torch.Tensor, point_adjacency_offsets: torch.Tensor,
                         box) -> BoxedCellGeometry:
    """Every Voronoi cell clipped to the axis-aligned ``box``: volume f64[N], centroid f64[N,3], nonempty bool[N],
    face_area f64[E] (the part of face (a,b) inside the box, aligned with ``point_adjacency``) and wall_area f64[N,6]
    (the part of each wall that bounds the cell; wall 2k is x_k >= lo_k, wall 2k+1 is x_k <= hi_k), in double.

    ``box`` is six numbers (lo, hi) as a sequence or tensor, or a [2,3] tensor; it is read on the host as doubles and
    need not contain the points.  Cell a is the intersection of the half-spaces of its row and of the six walls, so every
    cell is a bounded polytope and the cells of a Delaunay CSR partition the box: sum volume = the box's volume, and
    nothing is +inf.  A site outside the box still owns what its cell cuts out of the box.  An empty cell has volume 0,
    centroid NaN, areas 0 and nonempty False (nonempty is volume > 0; a flat cell may fall on either side by rounding);
    a cell with an empty row is the whole box.  Where a wall coincides with a bisector plane the row's face keeps the area
    and the wall gets 0.  Bit-reproducible; not differentiable (differentiable_cell_geometry_in_box is, and
    cell_geometry_in_box_grad is its operator).  Raises ValueError for a box that is not finite with
    lo < hi, and RuntimeError naming the cell like cell_geometry."""
    six = _box_six(box)
    return _run_geometry_in_box(*_prepare(points, point_adjacency, point_adjacency_offsets), six)[0]


def _run_geometry_in_box_grad(p, adj, off, bbox, six, volume, centroid, nonempty, grad_volume, grad_centroid):
    """grad_points f64[N,3]; one synchronisation, to read whether a row was refused."""
    grad = torch.empty((p.size(0), 3), dtype=torch.float64, device=p.device)
    _run_cells("cell_geometry_in_box_grad", "cell_box_grad", p, adj, off, bbox, volume, centroid, nonempty, grad_volume,
               grad_centroid, grad, six=six)
    return grad


def cell_geometry_in_box_grad(points: torch.Tensor, point_adjacency: torch.Tensor,
                              point_adjacency_offsets: torch.Tensor, box, geometry: BoxedCellGeometry, grad_volume,
                              grad_centroid) -> torch.Tensor:
    """f64[N,3]: the gradient with respect to ``points`` of  L = sum_a grad_volume[a] volume[a] + grad_centroid[a] .
    centroid[a]  over the non-empty cells, ``geometry`` being what cell_geometry_in_box returned for the same arguments.
    The box is fixed.

    The walls do not move, so only the row's faces carry a term, each by its part inside the box:
    grad p_a = sum over b in a's row of (1 / |p_b - p_a|) int_{F_ab n box} (phi_a - phi_b)(x) (x - p_a) dA  with
    phi_a(x) = grad_volume[a] + (grad_centroid[a] / volume[a]) . (x - centroid[a]), and phi_a = 0 for an empty cell:
    whatever arrives for it, NaN and inf included, is ignored, and so is its NaN centroid.  A face with an empty cell on
    either side carries no term (its part inside the box has area zero, or the empty cell is flat against a wall), so an
    empty cell's row is zero; a cell with an empty row gets zero; a site outside the box with a non-empty cell is an
    ordinary row.  Either upstream (f64 or f32, [N] and [N,3]) may be None.  The polygons are the forward's (the same
    plane list, clipping square and rule for coincident planes); where a wall coincides with a bisector plane the
    geometry is not differentiable, and the result follows that rule and stays finite.  A flat cell that rounding made
    ``nonempty`` has a volume of a few ulps, and ``grad_centroid / volume`` is as large as that makes it: masking such
    cells out of the loss is the caller's concern, as in the forward.  A gather over each site's own row,
    bit-reproducible: the exact gradient for a symmetric adjacency such as a Delaunay CSR; where a row omits a site
    that lists it, the omitted terms are dropped.  Raises ValueError for a bad box before any tensor is looked at,
    RuntimeError if ``geometry`` does not fit these points, and RuntimeError naming the cell like cell_geometry."""
    six = _box_six(box)
    p, adj, off, bbox = _prepare(points, point_adjacency, point_adjacency_offsets)
    n, dev = p.size(0), p.device
    volume, centroid, nonempty = (getattr(geometry, k, None) for k in ("volume", "centroid", "nonempty"))
    if (not all(isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev for t in (volume, centroid, nonempty))
            or volume.dtype != torch.float64 or volume.shape != (n,) or centroid.dtype != torch.float64
            or centroid.shape != (n, 3) or nonempty.dtype != torch.bool or nonempty.shape != (n,)):
        raise RuntimeError("geometry must be the BoxedCellGeometry cell_geometry_in_box returned for these points")
    return _run_geometry_in_box_grad(p, adj, off, bbox, six, volume.detach().contiguous(),
                                     centroid.detach().contiguous(), nonempty.contiguous().view(torch.uint8),
                                     _upstream("grad_volume", grad_volume, (n,), dev),
                                     _upstream("grad_centroid", grad_centroid, (n, 3), dev))


def _run_face_area_in_box_grad(p, adj, off, bbox, six, volume, centroid, nonempty, face_area, wall_area, grad_face_area,
                                grad_wall_area):
    """grad_points f64[N,3]; one synchronisation, to read whether a row was refused."""
    grad = torch.empty((p.size(0), 3), dtype=torch.float64, device=p.device)
    _run_cells("face_area_in_box_grad", "cell_box_area_grad", p, adj, off, bbox, volume, centroid, nonempty, face_area,
               wall_area, grad_face_area, grad_wall_area, grad, six=six, edge_workspace=True)
    return grad


def face_area_in_box_grad(points: torch.Tensor, point_adjacency: torch.Tensor, point_adjacency_offsets: torch.Tensor,
                          box, geometry: BoxedCellGeometry, grad_face_area=None, grad_wall_area=None) -> torch.Tensor:
    """f64[N,3]: the gradient with respect to ``points`` of  L = sum_s grad_face_area[s] face_area[s] + sum_{a,w}
    grad_wall_area[a,w] wall_area[a,w],  ``geometry`` being what cell_geometry_in_box returned for the same arguments.
    The box is fixed.

    In the box every face is a bounded polygon, so the gradient reaches every site, hull sites and sites outside the box
    included (face_area_grad only reaches faces between bounded cells).  An upstream counts where that slot's or wall's
    own forward area is > 0 and is ignored where it is exactly 0, NaN and inf included: an exactly empty cell has every
    area 0.  Face {a,b} weighs G_ab = g[a->b] + g[b->a].  A flat face changes its area through the in-plane motion of its
    edges, and every edge lies on a's own clipped polytope: a Voronoi edge, dual to a Delaunay triangle (a,b,c), adds
    l (lambda_b + lambda_c) (y - p_a)  as in face_area_grad, l and y the length and midpoint of the segment as the box
    clipped it; the trace of the bisector of (a,b) in wall w, which bounds face {a,b} and the two cells' parts of the
    wall, adds  (l (y - p_a) / |p_b - p_a|) [ -G_ab cot t + (gw[a,w] - gw[b,w]) / sin t ]  with cos t = n_w . (p_b - p_a)
    / |p_b - p_a| and n_w the wall's outward normal; edges between two walls do not move ("Point gradients of
    the face and wall areas in a box").  An empty row and an empty cell get a zero row.  Either upstream (f64 or f32,
    [E] and [N,6]) may be None, which is an all-zero upstream bit for bit.  The polygons are the forward's (the same plane
    list, clipping square and rule for coincident planes); where a wall coincides with a bisector plane the areas are not
    differentiable, and the result follows that rule and stays finite.  A gather over each site's own row with look-ups
    in its neighbours', bit-reproducible: the exact gradient for a symmetric adjacency such as a Delaunay CSR; where a
    mate slot or the slot b->c does not exist its weight is 0.  Raises ValueError for a bad box before any tensor is
    looked at, RuntimeError if ``geometry`` does not fit these points, and RuntimeError naming the cell like
    cell_geometry."""
    six = _box_six(box)
    p, adj, off, bbox = _prepare(points, point_adjacency, point_adjacency_offsets)
    n, e, dev = p.size(0), adj.numel(), p.device
    volume, centroid, nonempty, face_area, wall_area = (getattr(geometry, k, None) for k in (
        "volume", "centroid", "nonempty", "face_area", "wall_area"))
    if (not all(isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev
                for t in (volume, centroid, nonempty, face_area, wall_area))
            or volume.dtype != torch.float64 or volume.shape != (n,) or centroid.dtype != torch.float64
            or centroid.shape != (n, 3) or nonempty.dtype != torch.bool or nonempty.shape != (n,)
            or face_area.dtype != torch.float64 or face_area.shape != (e,) or wall_area.dtype != torch.float64
            or wall_area.shape != (n, 6)):
        raise RuntimeError("geometry must be the BoxedCellGeometry cell_geometry_in_box returned for these points")
    return _run_face_area_in_box_grad(p, adj, off, bbox, six, volume.detach().contiguous(),
                                      centroid.detach().contiguous(), nonempty.contiguous().view(torch.uint8),
                                      face_area.detach().contiguous(), wall_area.detach().contiguous(),
                                      _upstream("grad_face_area", grad_face_area, (e,), dev),
                                      _upstream("grad_wall_area", grad_wall_area, (n, 6), dev))


class _DifferentiableCellGeometryInBox(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, point_adjacency, point_adjacency_offsets, six, with_face_area):
        p, adj, off, bbox = _prepare(points, point_adjacency, point_adjacency_offsets)
        geo = _run_geometry_in_box(p, adj, off, bbox, six)[0]
        ctx.save_for_backward(p, adj, off, bbox, geo.volume, geo.centroid, geo.nonempty, geo.face_area, geo.wall_area)
        ctx.six = six
        ctx.points_dtype = points.dtype
        ctx.set_materialize_grads(False)      # an output the loss leaves out arrives as None and its operator is not run
        if with_face_area:
            ctx.mark_non_differentiable(geo.nonempty)
        else:
            ctx.mark_non_differentiable(geo.nonempty, geo.face_area, geo.wall_area)
        return geo.volume, geo.centroid, geo.nonempty, geo.face_area, geo.wall_area

    @staticmethod
    def backward(ctx, grad_volume, grad_centroid, _grad_nonempty, grad_face_area, grad_wall_area):
        p, adj, off, bbox, volume, centroid, nonempty, face_area, wall_area = ctx.saved_tensors
        n, e, dev = p.size(0), adj.numel(), p.device
        flags = nonempty.view(torch.uint8)
        grad = None
        if grad_volume is not None or grad_centroid is not None:
            grad = _run_geometry_in_box_grad(p, adj, off, bbox, ctx.six, volume, centroid, flags,
                                             _upstream("grad_volume", grad_volume, (n,), dev),
                                             _upstream("grad_centroid", grad_centroid, (n, 3), dev))
        if grad_face_area is not None or grad_wall_area is not None:
            part = _run_face_area_in_box_grad(p, adj, off, bbox, ctx.six, volume, centroid, flags, face_area, wall_area,
                                              _upstream("grad_face_area", grad_face_area, (e,), dev),
                                              _upstream("grad_wall_area", grad_wall_area, (n, 6), dev))
            grad = part if grad is None else grad + part
        if grad is None:
            grad = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        return grad.to(ctx.points_dtype), None, None, None, None


def differentiable_cell_geometry_in_box(points: torch.Tensor, point_adjacency: torch.Tensor,
                                        point_adjacency_offsets: torch.Tensor, box,
                                        face_area: bool = False) -> BoxedCellGeometry:
    """cell_geometry_in_box, bit for bit, with ``volume`` and ``centroid`` carrying autograd to ``points``
    (cell_geometry_in_box_grad: summed in double, returned in the dtype of ``points``); the box is fixed.  Every site
    owns a bounded cell here, hull sites and sites outside the box included, so mass terms sum density volume, Lloyd
    energies and equal-volume penalties reach all of them.  With ``face_area=True`` the face areas and the wall areas
    carry autograd as well (face_area_in_box_grad); the backward runs each operator only where something arrived and adds
    the two in double, cell_geometry_in_box_grad's result first.  By default ``nonempty``, ``face_area`` and ``wall_area``
    are not differentiable, and the backward is not run for an output the loss leaves out.  Mask the empty cells out of
    a loss (their centroid is NaN); what flows back for them is ignored."""
    six = _box_six(box)
    return BoxedCellGeometry(*_DifferentiableCellGeometryInBox.apply(points, point_adjacency, point_adjacency_offsets,
                                                                     six, bool(face_area)))


def cell_moments(points: torch.Tensor, point_adjacency: torch.Tensor, point_adjacency_offsets: torch.Tensor,
                 geometry: CellGeometry | None = None) -> CellMoments:
    """The second moments of every Voronoi cell, in double and relative to the site: ``site_moment`` f64[N,6] is
    int_{cell a} y y^T dy with y = x - p_a, stored as xx, yy, zz, xy, xz, yz, and ``central_moment`` f64[N,6] is
    site_moment - V_a m m^T with m = centroid[a] - p_a, the moment about the centroid.

    The trace of ``site_moment`` is the cell's centroidal-Voronoi energy int |x - p_a|^2 dx, and ``central_moment /
    volume`` the covariance of the uniform distribution on the cell: with the centroid as its mean, the cell's Gaussian.
    An unbounded cell gets NaN in all twelve.  ``geometry`` is what cell_geometry returned for the same arguments; when
    it is None cell_geometry runs first, and either way it comes back as the third field.  A gather over each site's own
    row, bit-reproducible; not differentiable (differentiable_cell_moments is, and cell_moments_grad is its operator).
    Raises RuntimeError naming the cell like cell_geometry."""
    p, adj, off, bbox = _prepare(points, point_adjacency, point_adjacency_offsets)
    n, dev = p.size(0), p.device
    if geometry is None:
        geometry = _run_geometry(p, adj, off, bbox)[0]
    volume, centroid, bounded = (getattr(geometry, k, None) for k in ("volume", "centroid", "bounded"))
    if (not all(isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev for t in (volume, centroid, bounded))
            or volume.dtype != torch.float64 or volume.shape != (n,) or centroid.dtype != torch.float64
            or centroid.shape != (n, 3) or bounded.dtype != torch.bool or bounded.shape != (n,)):
        raise RuntimeError("geometry must be the CellGeometry cell_geometry returned for these points")
    site, central = _run_moments(p, adj, off, bbox, volume.detach().contiguous(), centroid.detach().contiguous(),
                                 bounded.contiguous().view(torch.uint8))
    return CellMoments(site, central, geometry)


def _run_moments_in_box(p, adj, off, bbox, six, volume, centroid, nonempty):
    """(site f64[N,6], central f64[N,6]); one synchronisation, to read whether a cell was refused."""
    site = torch.empty((p.size(0), 6), dtype=torch.float64, device=p.device)
    central = torch.empty((p.size(0), 6), dtype=torch.float64, device=p.device)
    _run_cells("cell_moments_in_box", "cell_box_moments", p, adj, off, bbox, volume, centroid, nonempty, site, central,
               six=six)
    return site, central


def cell_moments_in_box(points: torch.Tensor, point_adjacency: torch.Tensor, point_adjacency_offsets: torch.Tensor,
                        box, geometry: BoxedCellGeometry | None = None) -> BoxedCellMoments:
    """The second moments of every Voronoi cell clipped to the axis-aligned ``box``, in double and relative to the site:
    ``site_moment`` f64[N,6] is the integral of y y^T over cell(a) n box with y = x - p_a, stored as xx, yy, zz, xy, xz,
    yz, and ``central_moment`` f64[N,6] is site_moment - V_a m m^T with m = centroid[a] - p_a, the moment about the
    centroid, V_a and the centroid being those of cell_geometry_in_box.

    Every cell is a bounded polytope in the box, so every site has its moments, hull sites and sites outside the box
    included (a site outside still owns what its cell cuts out of the box; the faces' pyramids over it are signed): the
    trace of ``site_moment`` summed over all sites is the centroidal-Voronoi energy of the box, and ``central_moment /
    volume`` is the covariance of the uniform distribution on the clipped cell, one Gaussian per non-empty cell.  For a
    site far outside the box V m m^T nearly cancels site_moment, and the central moment keeps fewer digits than
    site_moment does.  An exactly empty cell has site_moment 0; ``central_moment`` is NaN wherever ``nonempty`` is
    False; a cell with an empty row is the whole box.  ``box`` is as for cell_geometry_in_box.  ``geometry`` is what
    cell_geometry_in_box returned for the same arguments; when it is None cell_geometry_in_box runs first, and either way
    it comes back as the third field.  A gather over each site's own row, bit-reproducible.  Not differentiable itself:
    differentiable_cell_moments_in_box carries autograd to the points, and cell_moments_in_box_grad is its operator
    (the gradient with respect to the box is not built yet).  Raises ValueError for a box that is not finite with
    lo < hi before any tensor is looked at, RuntimeError if ``geometry`` does not fit these points, and
    RuntimeError naming the cell like cell_geometry."""
    six = _box_six(box)
    p, adj, off, bbox = _prepare(points, point_adjacency, point_adjacency_offsets)
    n, dev = p.size(0), p.device
    if geometry is None:
        geometry = _run_geometry_in_box(p, adj, off, bbox, six)[0]
    volume, centroid, nonempty = (getattr(geometry, k, None) for k in ("volume", "centroid", "nonempty"))
    if (not all(isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev for t in (volume, centroid, nonempty))
            or volume.dtype != torch.float64 or volume.shape != (n,) or centroid.dtype != torch.float64
            or centroid.shape != (n, 3) or nonempty.dtype != torch.bool or nonempty.shape != (n,)):
        raise RuntimeError("geometry must be the BoxedCellGeometry cell_geometry_in_box returned for these points")
    site, central = _run_moments_in_box(p, adj, off, bbox, six, volume.detach().contiguous(),
                                        centroid.detach().contiguous(), nonempty.contiguous().view(torch.uint8))
    return BoxedCellMoments(site, central, geometry)


def cell_surface(points: torch.Tensor, point_adjacency: torch.Tensor, point_adjacency_offsets: torch.Tensor,
                 inside: torch.Tensor):
    """(triangles f64[T,3,3], edge int64[T]): every face between a cell with ``inside`` set and a neighbour without, as
    a triangle fan wound so that its normal points out of the inside cell; ``edge`` is the adjacency slot each triangle
    came from.  The order is that of the adjacency slots: deterministic.  Vertices are not welded.

    Raises ValueError if ``inside`` selects an unbounded cell (its surface would not close)."""
    p, adj, off, bbox = _prepare(points, point_adjacency, point_adjacency_offsets)
    n, e, dev = p.size(0), adj.numel(), p.device
    if not inside.is_cuda or inside.device != dev or inside.dtype != torch.bool or inside.shape != (n,):
        raise RuntimeError("inside must be a bool[N] CUDA tensor on the device of points")
    geo, face_vertices = _run_geometry(p, adj, off, bbox)
    if bool((inside & ~geo.bounded).any()):
        raise ValueError("cell_surface: inside selects an unbounded cell")
    lib = _lib.load()
    mask = inside.contiguous().view(torch.uint8)
    counts = torch.zeros(e, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.rf_cell_surface_count(n, _ptr(adj), _ptr(off), e, _ptr(mask), _ptr(face_vertices), _ptr(counts),
                                             _stream(dev)))
    slots = torch.nonzero(counts).reshape(-1)                      # ascending adjacency slots
    ends = torch.cumsum(counts[slots], 0, dtype=torch.int64)
    total = int(ends[-1]) if slots.numel() else 0
    begins = (ends - counts[slots]).contiguous()
    triangles = torch.empty((total, 3, 3), dtype=torch.float64, device=dev)
    edge = torch.empty(total, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.rf_cell_surface_emit(_ptr(p), n, _ptr(adj), _ptr(off), e, _ptr(bbox), _ptr(face_vertices),
                                            _ptr(slots), _ptr(begins), slots.numel(), _ptr(triangles), _ptr(edge),
                                            _stream(dev)))
    return triangles, edge


def _upstream(name, t, shape, device):
    if t is None:
        return None
    if not t.is_cuda or t.device != device or tuple(t.shape) != shape or not t.dtype.is_floating_point:
        raise RuntimeError(f"{name} must be a floating-point CUDA tensor of shape {list(shape)} on the device of points")
    return t.detach().to(torch.float64).contiguous()


def _run_geometry_grad(p, adj, off, bbox, volume, centroid, bounded, grad_volume, grad_centroid):
    """grad_points f64[N,3]; one synchronisation, to read whether a row was refused."""
    grad = torch.empty((p.size(0), 3), dtype=torch.float64, device=p.device)
    _run_cells("cell_geometry_grad", "cell_geometry_grad", p, adj, off, bbox, volume, centroid, bounded, grad_volume,
               grad_centroid, grad)
    return grad


def cell_geometry_grad(points: torch.Tensor, point_adjacency: torch.Tensor, point_adjacency_offsets: torch.Tensor,
                       geometry: CellGeometry, grad_volume, grad_centroid) -> torch.Tensor:
    """f64[N,3]: the gradient with respect to ``points`` of  L = sum_a grad_volume[a] volume[a] + grad_centroid[a] .
    centroid[a]  over the bounded cells, ``geometry`` being what cell_geometry returned for the same arguments.

    grad p_a = sum over b in a's row of (1 / |p_b - p_a|) int_{F_ab} (phi_a - phi_b)(x) (x - p_a) dA  with
    phi_a(x) = grad_volume[a] + (grad_centroid[a] / volume[a]) . (x - centroid[a]), and phi_a = 0 for an unbounded cell:
    whatever arrives for it, NaN and inf included, is ignored.  Either upstream (f64 or f32, [N] and [N,3]) may be None.
    A gather over each site's own row, bit-reproducible: the exact gradient for a symmetric adjacency such as a
    Delaunay CSR; where a row omits a site that lists it, the omitted terms are dropped.  Face areas are not
    differentiated.  Raises RuntimeError naming the cell like cell_geometry."""
    p, adj, off, bbox = _prepare(points, point_adjacency, point_adjacency_offsets)
    n, dev = p.size(0), p.device
    volume, centroid, bounded = geometry.volume, geometry.centroid, geometry.bounded
    if (not volume.is_cuda or volume.device != dev or volume.dtype != torch.float64 or volume.shape != (n,)
            or centroid.device != dev or centroid.dtype != torch.float64 or centroid.shape != (n, 3)
            or bounded.device != dev or bounded.dtype != torch.bool or bounded.shape != (n,)):
        raise RuntimeError("geometry must be the CellGeometry cell_geometry returned for these points")
    return _run_geometry_grad(p, adj, off, bbox, volume.detach().contiguous(), centroid.detach().contiguous(),
                              bounded.contiguous().view(torch.uint8), _upstream("grad_volume", grad_volume, (n,), dev),
                              _upstream("grad_centroid", grad_centroid, (n, 3), dev))


def _run_face_area_grad(p, adj, off, bbox, face_area, grad_face_area):
    """grad_points f64[N,3]; one synchronisation, to read whether a row was refused."""
    grad = torch.empty((p.size(0), 3), dtype=torch.float64, device=p.device)
    _run_cells("face_area_grad", "face_area_grad", p, adj, off, bbox, face_area, grad_face_area, grad,
               edge_workspace=True)
    return grad


def face_area_grad(points: torch.Tensor, point_adjacency: torch.Tensor, point_adjacency_offsets: torch.Tensor,
                   geometry: CellGeometry, grad_face_area: torch.Tensor) -> torch.Tensor:
    """f64[N,3]: the gradient with respect to ``points`` of  L = sum_s grad_face_area[s] face_area[s]  over the adjacency
    slots whose area is finite, ``geometry`` being what cell_geometry returned for the same arguments.

    Face {a,b} weighs G_ab = g[a->b] + g[b->a] (each where that slot's area is finite; what arrives for a slot of area
    +inf, NaN and inf included, is ignored, and so is a slot of area exactly 0, which the forward clipped away).  A
    flat face changes its area through the in-plane motion of its edges, and every finite Voronoi edge of cell a, dual to
    a Delaunay triangle (a,b,c), adds  l (lambda_b + lambda_c) (y - p_a)  to grad p_a, l and y the edge's length and
    midpoint and lambda from G_ab, G_ac, G_bc and the triangle ("Point gradients of the face areas").  A
    gather over each site's own row with one look-up in a neighbour's, bit-reproducible: the exact gradient for a
    symmetric adjacency such as a Delaunay CSR; where a mate slot or the slot b->c does not exist its weight is 0.
    ``grad_face_area`` is a floating-point [E] CUDA tensor.  Raises RuntimeError naming the cell like cell_geometry."""
    p, adj, off, bbox = _prepare(points, point_adjacency, point_adjacency_offsets)
    e, dev = adj.numel(), p.device
    face_area = getattr(geometry, "face_area", None)
    if (not isinstance(face_area, torch.Tensor) or not face_area.is_cuda or face_area.device != dev
            or face_area.dtype != torch.float64 or face_area.shape != (e,)):
        raise RuntimeError("geometry must be the CellGeometry cell_geometry returned for these points")
    if grad_face_area is None:
        raise RuntimeError(f"grad_face_area must be a floating-point CUDA tensor of shape {[e]} on the device of points")
    return _run_face_area_grad(p, adj, off, bbox, face_area.detach().contiguous(),
                               _upstream("grad_face_area", grad_face_area, (e,), dev))


class _DifferentiableCellGeometry(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, point_adjacency, point_adjacency_offsets, with_face_area):
        p, adj, off, bbox = _prepare(points, point_adjacency, point_adjacency_offsets)
        geo = _run_geometry(p, adj, off, bbox)[0]
        ctx.save_for_backward(p, adj, off, bbox, geo.volume, geo.centroid, geo.bounded, geo.face_area)
        ctx.points_dtype = points.dtype
        ctx.set_materialize_grads(False)      # an output the loss leaves out arrives as None and its operator is not run
        if with_face_area:
            ctx.mark_non_differentiable(geo.bounded)
        else:
            ctx.mark_non_differentiable(geo.bounded, geo.face_area)
        return geo.volume, geo.centroid, geo.bounded, geo.face_area

    @staticmethod
    def backward(ctx, grad_volume, grad_centroid, _grad_bounded, grad_face_area):
        p, adj, off, bbox, volume, centroid, bounded, face_area = ctx.saved_tensors
        n, e, dev = p.size(0), adj.numel(), p.device
        grad = None
        if grad_volume is not None or grad_centroid is not None:
            grad = _run_geometry_grad(p, adj, off, bbox, volume, centroid, bounded.view(torch.uint8),
                                      _upstream("grad_volume", grad_volume, (n,), dev),
                                      _upstream("grad_centroid", grad_centroid, (n, 3), dev))
        if grad_face_area is not None:
            part = _run_face_area_grad(p, adj, off, bbox, face_area, _upstream("grad_face_area", grad_face_area, (e,), dev))
            grad = part if grad is None else grad + part
        if grad is None:
            grad = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        return grad.to(ctx.points_dtype), None, None, None


def _run_moments(p, adj, off, bbox, volume, centroid, flags):
    """(site f64[N,6], central f64[N,6]); one synchronisation, to read whether a cell was refused."""
    site = torch.empty((p.size(0), 6), dtype=torch.float64, device=p.device)
    central = torch.empty((p.size(0), 6), dtype=torch.float64, device=p.device)
    _run_cells("cell_moments", "cell_moments", p, adj, off, bbox, volume, centroid, flags, site, central)
    return site, central


def _run_moments_grad(p, adj, off, bbox, volume, centroid, bounded, grad_site_moment, grad_central_moment):
    """grad_points f64[N,3]; one synchronisation, to read whether a row was refused."""
    grad = torch.empty((p.size(0), 3), dtype=torch.float64, device=p.device)
    _run_cells("cell_moments_grad", "cell_moments_grad", p, adj, off, bbox, volume, centroid, bounded,
               grad_site_moment, grad_central_moment, grad)
    return grad


def cell_moments_grad(points: torch.Tensor, point_adjacency: torch.Tensor, point_adjacency_offsets: torch.Tensor,
                      geometry: CellGeometry, grad_site_moment=None, grad_central_moment=None) -> torch.Tensor:
    """f64[N,3]: the gradient with respect to ``points`` of  L = sum_a <grad_site_moment[a], site_moment[a]> +
    <grad_central_moment[a], central_moment[a]>  over the bounded cells, each bracket the plain sum over the six stored
    numbers (xx, yy, zz, xy, xz, yz), ``geometry`` being what cell_geometry returned for the same arguments.

    With G_a and H_a the symmetric matrices of the two upstreams (the diagonal as it is, half of each off-diagonal number
    on both sides) and Psi_a(x) = (x - p_a)^T G_a (x - p_a) + (x - c_a)^T H_a (x - c_a), Psi_a = 0 for an unbounded cell
    (whatever arrives for it, NaN and inf included, is ignored),
    grad p_a = sum over b in a's row of (1 / |p_b - p_a|) int_{F_ab} (Psi_a - Psi_b)(x) (x - p_a) dA  -  2 V_a G_a
    (c_a - p_a); the central moment has no direct term, because the first moment about the centroid vanishes.  Either
    upstream (f64 or f32, [N,6]) may be None.  A gather over each site's own row, bit-reproducible: the exact gradient
    for a symmetric adjacency such as a Delaunay CSR; where a row omits a site that lists it, the omitted terms are
    dropped.  Raises RuntimeError naming the cell like cell_geometry."""
    p, adj, off, bbox = _prepare(points, point_adjacency, point_adjacency_offsets)
    n, dev = p.size(0), p.device
    volume, centroid, bounded = (getattr(geometry, k, None) for k in ("volume", "centroid", "bounded"))
    if (not all(isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev for t in (volume, centroid, bounded))
            or volume.dtype != torch.float64 or volume.shape != (n,) or centroid.dtype != torch.float64
            or centroid.shape != (n, 3) or bounded.dtype != torch.bool or bounded.shape != (n,)):
        raise RuntimeError("geometry must be the CellGeometry cell_geometry returned for these points")
    return _run_moments_grad(p, adj, off, bbox, volume.detach().contiguous(), centroid.detach().contiguous(),
                             bounded.contiguous().view(torch.uint8),
                             _upstream("grad_site_moment", grad_site_moment, (n, 6), dev),
                             _upstream("grad_central_moment", grad_central_moment, (n, 6), dev))


class _DifferentiableCellMoments(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, point_adjacency, point_adjacency_offsets):
        p, adj, off, bbox = _prepare(points, point_adjacency, point_adjacency_offsets)
        geo = _run_geometry(p, adj, off, bbox)[0]
        site, central = _run_moments(p, adj, off, bbox, geo.volume, geo.centroid, geo.bounded.view(torch.uint8))
        ctx.save_for_backward(p, adj, off, bbox, geo.volume, geo.centroid, geo.bounded)
        ctx.points_dtype = points.dtype
        ctx.set_materialize_grads(False)      # an output the loss leaves out arrives as None and its operator is not run
        ctx.mark_non_differentiable(geo.bounded, geo.face_area)
        return site, central, geo.volume, geo.centroid, geo.bounded, geo.face_area

    @staticmethod
    def backward(ctx, grad_site, grad_central, grad_volume, grad_centroid, _grad_bounded, _grad_face_area):
        p, adj, off, bbox, volume, centroid, bounded = ctx.saved_tensors
        n, dev = p.size(0), p.device
        flags = bounded.view(torch.uint8)
        grad = None
        if grad_site is not None or grad_central is not None:
            grad = _run_moments_grad(p, adj, off, bbox, volume, centroid, flags,
                                     _upstream("grad_site_moment", grad_site, (n, 6), dev),
                                     _upstream("grad_central_moment", grad_central, (n, 6), dev))
        if grad_volume is not None or grad_centroid is not None:
            part = _run_geometry_grad(p, adj, off, bbox, volume, centroid, flags,
                                      _upstream("grad_volume", grad_volume, (n,), dev),
                                      _upstream("grad_centroid", grad_centroid, (n, 3), dev))
            grad = part if grad is None else grad + part
        if grad is None:
            grad = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        return grad.to(ctx.points_dtype), None, None


def differentiable_cell_moments(points: torch.Tensor, point_adjacency: torch.Tensor,
                                point_adjacency_offsets: torch.Tensor) -> CellMoments:
    """cell_moments, bit for bit, with ``site_moment`` and ``central_moment`` carrying autograd to ``points``
    (cell_moments_grad), and ``geometry.volume`` and ``geometry.centroid`` as in differentiable_cell_geometry
    (cell_geometry_grad): ``central_moment / volume[:, None]``, the covariance, and the trace of ``site_moment``, the
    centroidal-Voronoi energy, are differentiable end to end.  The backward runs each operator only where something
    arrived and adds the two in double; the result is returned in the dtype of ``points``.  ``geometry.bounded`` and
    ``geometry.face_area`` are not differentiable.  Mask the unbounded cells out of a loss (their moments and centroid
    are NaN and their volume +inf); what flows back for them is ignored."""
    site, central, *geo = _DifferentiableCellMoments.apply(points, point_adjacency, point_adjacency_offsets)
    return CellMoments(site, central, CellGeometry(*geo))


def differentiable_cell_geometry(points: torch.Tensor, point_adjacency: torch.Tensor,
                                 point_adjacency_offsets: torch.Tensor, face_area: bool = False) -> CellGeometry:
    """cell_geometry, bit for bit, with ``volume`` and ``centroid`` carrying autograd to ``points`` (cell_geometry_grad:
    summed in double, returned in the dtype of ``points``).  With ``face_area=True`` the face areas carry autograd as well
    (face_area_grad); the backward runs each operator only where something arrived and adds the two in double.  By
    default ``bounded`` and ``face_area`` are not differentiable.  Mask the unbounded cells and faces out of a loss (their
    volume and area are +inf and their centroid NaN); what flows back for them is ignored."""
    return CellGeometry(*_DifferentiableCellGeometry.apply(points, point_adjacency, point_adjacency_offsets,
                                                           bool(face_area)))


def _run_moments_in_box_grad(p, adj, off, bbox, six, volume, centroid, nonempty, grad_site_moment, grad_central_moment,
                             grad_volume, grad_centroid):
    """grad_points f64[N,3]; one launch of the fused operator and one synchronisation, to read whether a row was
    refused."""
    grad = torch.empty((p.size(0), 3), dtype=torch.float64, device=p.device)
    _run_cells("cell_moments_in_box_grad", "cell_box_moments_grad", p, adj, off, bbox, volume, centroid, nonempty,
               grad_site_moment, grad_central_moment, grad_volume, grad_centroid, grad, six=six)
    return grad


def cell_moments_in_box_grad(points: torch.Tensor, point_adjacency: torch.Tensor, point_adjacency_offsets: torch.Tensor,
                             box, geometry: BoxedCellGeometry, grad_site_moment=None, grad_central_moment=None,
                             grad_volume=None, grad_centroid=None) -> torch.Tensor:
    """f64[N,3]: the gradient with respect to ``points`` of  L = sum_a <grad_site_moment[a], site_moment[a]> +
    <grad_central_moment[a], central_moment[a]> + grad_volume[a] volume[a] + grad_centroid[a] . centroid[a]  over the
    non-empty cells of cell_moments_in_box, each bracket the plain sum over the six stored numbers (xx, yy, zz, xy, xz,
    yz), ``geometry`` being what cell_geometry_in_box returned for the same arguments.  The box is fixed.  One launch
    for all four upstreams: a loss that mixes moments with volume or centroid terms clips every face once.

    With G_a and H_a the symmetric matrices of the two moment upstreams (the diagonal as it is, half of each off-diagonal
    number on both sides) and Psi_a(x) = (x - p_a)^T G_a (x - p_a) + (x - c_a)^T H_a (x - c_a) + grad_volume[a] +
    (grad_centroid[a] / volume[a]) . (x - c_a), Psi_a = 0 for an empty cell (whatever arrives for it, NaN and inf
    included, is ignored, and so is its NaN centroid),
    grad p_a = sum over b in a's row of (1 / |p_b - p_a|) int_{F_ab n box} (Psi_a - Psi_b)(x) (x - p_a) dA  -  2 V_a G_a
    (c_a - p_a).  The walls do not move, so only the row's faces carry a boundary term, each by its part inside the box.
    The last, direct term is the site moment's alone (the central moment has none, because c_a is the centroid of the
    clipped cell, nor have the volume and the centroid) and is there whenever the cell is non-empty, also for an empty
    row: that cell is the whole box, and grad p_a = -2 V_box G_a (centre - p_a).  A face with an empty cell on either side
    carries no term, so an empty cell's row is zero; a site outside the box with a non-empty cell is an ordinary row.
    Any of the four upstreams (f64 or f32; [N,6], [N,6], [N], [N,3]) may be None.  The polygons are the forward's (the
    same plane list, clipping square and rule for coincident planes); where a wall coincides with a bisector plane the
    geometry is not differentiable, and the result follows that rule and stays finite.  A flat cell that rounding made
    ``nonempty`` has a volume of a few ulps, and ``grad_centroid / volume`` is as large as that makes it: masking such
    cells out of the loss is the caller's concern, as in the forward.  A gather over each site's own row,
    bit-reproducible: the exact gradient for a symmetric adjacency such as a Delaunay CSR; where a row omits a site that
    lists it, the omitted terms are dropped.  Raises ValueError for a bad box before any tensor is looked at, RuntimeError
    if ``geometry`` does not fit these points, and RuntimeError naming the cell like cell_geometry."""
    six = _box_six(box)
    p, adj, off, bbox = _prepare(points, point_adjacency, point_adjacency_offsets)
    n, dev = p.size(0), p.device
    volume, centroid, nonempty = (getattr(geometry, k, None) for k in ("volume", "centroid", "nonempty"))
    if (not all(isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev for t in (volume, centroid, nonempty))
            or volume.dtype != torch.float64 or volume.shape != (n,) or centroid.dtype != torch.float64
            or centroid.shape != (n, 3) or nonempty.dtype != torch.bool or nonempty.shape != (n,)):
        raise RuntimeError("geometry must be the BoxedCellGeometry cell_geometry_in_box returned for these points")
    return _run_moments_in_box_grad(p, adj, off, bbox, six, volume.detach().contiguous(),
                                    centroid.detach().contiguous(), nonempty.contiguous().view(torch.uint8),
                                    _upstream("grad_site_moment", grad_site_moment, (n, 6), dev),
                                    _upstream("grad_central_moment", grad_central_moment, (n, 6), dev),
                                    _upstream("grad_volume", grad_volume, (n,), dev),
                                    _upstream("grad_centroid", grad_centroid, (n, 3), dev))


class _DifferentiableCellMomentsInBox(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, point_adjacency, point_adjacency_offsets, six):
        p, adj, off, bbox = _prepare(points, point_adjacency, point_adjacency_offsets)
        geo = _run_geometry_in_box(p, adj, off, bbox, six)[0]
        site, central = _run_moments_in_box(p, adj, off, bbox, six, geo.volume, geo.centroid,
                                            geo.nonempty.view(torch.uint8))
        ctx.save_for_backward(p, adj, off, bbox, geo.volume, geo.centroid, geo.nonempty)
        ctx.six = six
        ctx.points_dtype = points.dtype
        ctx.set_materialize_grads(False)      # an output the loss leaves out arrives as None and its operator is not run
        ctx.mark_non_differentiable(geo.nonempty, geo.face_area, geo.wall_area)
        return site, central, geo.volume, geo.centroid, geo.nonempty, geo.face_area, geo.wall_area

    @staticmethod
    def backward(ctx, grad_site, grad_central, grad_volume, grad_centroid, _grad_nonempty, _grad_face_area,
                 _grad_wall_area):
        p, adj, off, bbox, volume, centroid, nonempty = ctx.saved_tensors
        n, dev = p.size(0), p.device
        flags = nonempty.view(torch.uint8)
        gv = _upstream("grad_volume", grad_volume, (n,), dev)
        gc = _upstream("grad_centroid", grad_centroid, (n, 3), dev)
        if grad_site is not None or grad_central is not None:      # one launch with every upstream that is present
            grad = _run_moments_in_box_grad(p, adj, off, bbox, ctx.six, volume, centroid, flags,
                                            _upstream("grad_site_moment", grad_site, (n, 6), dev),
                                            _upstream("grad_central_moment", grad_central, (n, 6), dev), gv, gc)
        elif gv is not None or gc is not None:
            grad = _run_geometry_in_box_grad(p, adj, off, bbox, ctx.six, volume, centroid, flags, gv, gc)
        else:
            grad = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        return grad.to(ctx.points_dtype), None, None, None


def differentiable_cell_moments_in_box(points: torch.Tensor, point_adjacency: torch.Tensor,
                                       point_adjacency_offsets: torch.Tensor, box) -> BoxedCellMoments:
    """cell_moments_in_box, bit for bit, with ``site_moment``, ``central_moment``, ``geometry.volume`` and
    ``geometry.centroid`` carrying autograd to ``points``; the box is fixed.  Every site owns a bounded cell here, hull
    sites and sites outside the box included: the trace of ``site_moment`` summed over all sites, the centroidal-Voronoi
    energy of the whole box, and ``central_moment / volume[:, None]``, the covariance, are differentiable end to end and
    reach every site.  When a moment upstream is present the backward is ONE launch of cell_moments_in_box_grad with
    every upstream that is present, so a loss that mixes moments with volume or centroid terms pays for the clipping
    once; with only volume and centroid upstreams it is cell_geometry_in_box_grad, bit for bit what
    differentiable_cell_geometry_in_box gives; for an output the loss leaves out nothing is run.  Summed in double,
    returned in the dtype of ``points``.  ``geometry.nonempty``, ``geometry.face_area`` and ``geometry.wall_area`` are not
    differentiable.  Mask the empty cells out of a loss (their central moment and centroid are NaN); what flows back for
    them is ignored."""
    six = _box_six(box)
    site, central, *geo = _DifferentiableCellMomentsInBox.apply(points, point_adjacency, point_adjacency_offsets, six)
    return BoxedCellMoments(site, central, BoxedCellGeometry(*geo))
