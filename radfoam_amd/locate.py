"""The field of a per-site value interpolated linearly over the Delaunay tetrahedra, at any point ("Point
location and interpolation").

  locate_tets        the tetrahedron that contains every query: a walk over ``tet_adjacency`` with exact face signs
  interpolate        value, barycentric weights and spatial gradient of the field at located queries; ``value`` carries
                     autograd to ``values``, ``points`` and ``queries``
  interpolate_grad   its backward operator

csrc/rf_locate.hpp states the definitions once (the face signs, the step, the faults, the order of every operation of the
interpolation and of its backward); the kernels of csrc/rf_locate.hip behind the C-ABI of include/radfoam_hip_locate.h,
the host build of the tests and the numpy / torch restatement here share them to the letter.  The sort of the backward's
gather is torch on the device.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _lib
from .scene_ops import _ptr, _stream
from .segments import _choose_backend

_HULL = 0xFFFFFFFF
_MAX_CHANNELS = 8     # rf::locate::kMaxChannels
# rf::locate::Fault
_BAD_ROW, _BAD_ADJACENCY, _FLAT_ROW, _BAD_START, _HOP_CAP = range(5)
_INDEX_DTYPES = (torch.uint32, torch.int32, torch.int64)


class TetLocation(NamedTuple):
    tet: torch.Tensor    # int64[...]; the row of tets whose closed tetrahedron holds the query, -1 outside the hull
    hops: torch.Tensor   # int32[...]; the faces the walk crossed


class FieldSamples(NamedTuple):
    value: torch.Tensor      # f64[...] or [...,C]
    weights: torch.Tensor    # f64[...,4]; the barycentric weights of the row's four sites, detached
    gradient: torch.Tensor   # f64[...,3] or [...,C,3]; the spatial gradient, constant per tetrahedron, detached


def _fault_code(kind, row):
    return -2 - (kind + 8 * row)


# ---- checks -----------------------------------------------------------------------------------------------------------

def _check_points(points):
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.size(-1) != 3 or not points.dtype.is_floating_point:
        raise RuntimeError("points must be a floating-point [N,3] tensor")
    if points.size(0) >= 2 ** 31:
        raise RuntimeError("more than 2^31 points")


def _check_table(name, points, table, rows=None):
    if (not isinstance(table, torch.Tensor) or table.dtype not in _INDEX_DTYPES or table.dim() != 2 or table.size(-1) != 4
            or table.device != points.device or (rows is not None and table.size(0) != rows)):
        raise RuntimeError(f"{name} must be a uint32, int32 or int64 [T,4] tensor on the device of points")
    if table.size(0) >= 2 ** 30:
        raise RuntimeError("2^30 tetrahedra or more")


def _check_queries(points, queries):
    if (not isinstance(queries, torch.Tensor) or queries.dim() < 1 or queries.size(-1) != 3
            or not queries.dtype.is_floating_point or queries.device != points.device):
        raise RuntimeError("queries must be a floating-point [...,3] tensor on the device of points")
    if queries.numel() // 3 > 2 ** 30:
        raise RuntimeError("more than 2^30 queries")


def _kernel_table(t):
    """the table as the kernels take it: contiguous, 16-byte aligned, uint32 as its int32 words"""
    t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone()
    return t.view(torch.int32) if t.dtype == torch.uint32 else t


def _int64(t):
    return t if t.dtype == torch.int64 else t.to(torch.int64)


# ---- the walk ---------------------------------------------------------------------------------------------------------

def _orient_signs(pi, pa, pb, pc):
    """numpy int64[M]: the exact sign of det[a - i; b - i; c - i] of float32 [M,3] points: the double determinant where it
    exceeds the forward error bound of tets.canonical_rows, Fractions (tets._exact_sign) below"""
    import numpy as np
    from .tets import _exact_sign
    i64 = pi.astype(np.float64)
    a, b, c = pa.astype(np.float64) - i64, pb.astype(np.float64) - i64, pc.astype(np.float64) - i64
    terms = np.stack([a[:, 0] * b[:, 1] * c[:, 2], -a[:, 0] * b[:, 2] * c[:, 1], -a[:, 1] * b[:, 0] * c[:, 2],
                      a[:, 1] * b[:, 2] * c[:, 0], a[:, 2] * b[:, 0] * c[:, 1], -a[:, 2] * b[:, 1] * c[:, 0]], 1)
    det, perm = terms.sum(1), np.abs(terms).sum(1)
    sign = np.sign(det).astype(np.int64)
    for m in np.nonzero(~(np.abs(det) > 4.0e-15 * perm))[0]:
        sign[m] = _exact_sign(np.stack([pi[m], pa[m], pb[m], pc[m]]))
    return sign


def _face_signs(p, q):
    """numpy int64[M,4]: sigma_j of float32 rows p [M,4,3] and queries q [M,3], in the arrangement of rf_locate.hpp"""
    import numpy as np
    p0, p1, p2, p3 = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    return np.stack([_orient_signs(q, p1, p2, p3), _orient_signs(q, p0, p3, p2), _orient_signs(q, p0, p1, p3),
                     _orient_signs(q, p1, p0, p2)], 1)


def _walk_numpy(pts, tets, adjacency, queries, start, max_hops):
    """(tet int64[Q] with the fault codes of rf_locate.hpp, hops int32[Q]) of numpy float32 pts [N,3] and queries [Q,3],
    int64 tets / adjacency [T,4] (hull: -1 or 0xFFFFFFFF) and int64 start [Q]: rf::locate::walk, all queries at once"""
    import numpy as np
    n, nt, nq = len(pts), len(tets), len(queries)
    tet, hops = np.full(nq, -1, dtype=np.int64), np.zeros(nq, dtype=np.int32)
    finite = np.isfinite(queries).all(1)
    bad = finite & ((start < 0) | (start >= nt))
    tet[bad] = _fault_code(_BAD_START, 0)
    active = np.nonzero(finite & ~bad)[0]
    cur, crossed = start[active].astype(np.int64), np.zeros(len(active), dtype=np.int64)

    def settle(which, result):
        nonlocal active, cur, crossed
        tet[active[which]], hops[active[which]] = result, crossed[which]
        active, cur, crossed = active[~which], cur[~which], crossed[~which]

    while len(active):
        rows = tets[cur]
        outside = ~((rows >= 0) & (rows < n)).all(1)
        if outside.any():
            settle(outside, _fault_code(_BAD_ROW, cur[outside]))
            continue
        sigma = _face_signs(pts[rows], queries[active])
        inside = ~(sigma < 0).any(1)
        if inside.any():
            flat = (sigma[inside] == 0).all(1)
            settle(inside, np.where(flat, _fault_code(_FLAT_ROW, cur[inside]), cur[inside]))
            continue
        entry = adjacency[cur, (sigma < 0).argmax(1)]
        hull = (entry == -1) | (entry == _HULL)
        stop = hull | (entry < 0) | (entry >= 4 * nt) | (crossed >= max_hops)
        if stop.any():
            e = entry[stop]
            code = np.where(hull[stop], -1, np.where((e < 0) | (e >= 4 * nt), _fault_code(_BAD_ADJACENCY, cur[stop]),
                                                       _fault_code(_HOP_CAP, cur[stop])))
            settle(stop, code)
            continue
        cur, crossed = entry >> 2, crossed + 1
    return tet, hops


def _walk_host(p, tets, adjacency, q, start, max_hops):
    import numpy as np
    to64 = lambda t: _int64(t).numpy()
    s = np.zeros(q.size(0), dtype=np.int64) if start is None else _int64(start).numpy()
    tet, hops = _walk_numpy(p.numpy(), to64(tets), to64(adjacency), q.numpy(), s, max_hops)
    return torch.from_numpy(tet), torch.from_numpy(hops)


def _walk_hip(p, tets, adjacency, q, start, max_hops):
    """(tet, hops, flags int32[2]) on the device; nothing synchronises"""
    n, nt, nq, dev = p.size(0), tets.size(0), q.size(0), p.device
    if tets.element_size() != adjacency.element_size():
        tets, adjacency = _int64(tets), _int64(adjacency)
    tets, adjacency = _kernel_table(tets), _kernel_table(adjacency)
    s = None if start is None else _int64(start).contiguous()
    tet = torch.empty(nq, dtype=torch.int64, device=dev)
    hops = torch.empty(nq, dtype=torch.int32, device=dev)
    flags = torch.zeros(2, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().rf_locate_walk(_ptr(p), n, _ptr(tets), _ptr(adjacency), tets.element_size(), nt, _ptr(q),
                                              None if s is None else _ptr(s), nq, max_hops, _ptr(tet), _ptr(hops),
                                              _ptr(flags), _stream(dev)))
    return tet, hops, flags


def _fault_error(tet, start, n, nt, max_hops):
    """the RuntimeError of the first faulted query (found on this path only)"""
    k = int(torch.nonzero(tet < -1)[0])
    code = -2 - int(tet[k])
    kind, row = code & 7, code >> 3
    what = {_BAD_ROW: f"tetrahedron {row} has a corner index outside [0, {n})",
            _BAD_ADJACENCY: f"tetrahedron {row} has an adjacency entry that is neither the hull word nor below {4 * nt}",
            _FLAT_ROW: f"tetrahedron {row} is flat (all four face determinants of the query are zero)",
            _BAD_START: f"its start {0 if start is None else int(start[k])} is outside [0, {nt})",
            _HOP_CAP: f"its walk would cross more than max_hops = {max_hops} faces (at tetrahedron {row}): the mesh is "
                      "stale, not Delaunay or negatively oriented, or max_hops is too small"}[kind]
    return RuntimeError(f"locate_tets: query {k}: {what}")


def locate_tets(points: torch.Tensor, tets: torch.Tensor, tet_adjacency: torch.Tensor, queries: torch.Tensor,
                start=None, max_hops=None) -> TetLocation:
    """The tetrahedron of ``tets`` (uint32, int32 or int64 [T,4], positively oriented rows as delaunay_tets /
    Triangulation.tets() give them) that contains every query (float32 [...,3]), by walking over ``tet_adjacency``
    ([T,4]: 4 t' + j' across the face opposite corner j, 0xFFFFFFFF -- or -1 -- on the hull).

    At a tetrahedron the walk takes the exact sign of the four face determinants (the row's determinant with corner j
    replaced by the query; the predicate of the triangulation, csrc/rf_star.hpp: fp64 with an error bound, 384-bit
    integers below it), crosses the face of the lowest corner with a negative sign, and stops where none is negative:
    ``tet`` (int64[...]) is that row, ``hops`` (int32[...]) the faces crossed.  Leaving through a hull face gives -1;
    so does a query with a coordinate that is not finite (0 hops, no walk).

    ``start`` (uint32, int32 or int64 [...]): the row every walk starts at, in [0, T).  None starts every walk at row 0,
    which is correct and slow (the walk crosses the mesh): meant for tests and small meshes; Triangulation.locate starts
    at a tetrahedron of the nearest site.  The result depends on the start only where the query lies on a shared face,
    edge or vertex; with the same start it is the same on every backend, bit for bit.

    Guaranteed: a returned ``tet >= 0`` contains its query exactly (closed tetrahedron), whatever the tables hold.  -1 is
    only right for conforming input: positive rows that triangulate a convex hull.  On a strictly Delaunay mesh the walk
    ends (every step lowers the query's power with respect to the circumsphere).  A walk that would cross more than
    ``max_hops`` faces (default min(T, 2^20)) raises RuntimeError naming the first such query: that is how a stale,
    non-Delaunay or negatively oriented mesh ends.  So do, naming the first offender met by a walk: a start outside
    [0, T), a corner index outside [0, N), an adjacency entry that is neither the hull word nor below 4T, and a flat row
    whose plane holds the query.  The exactness has the predicate's documented limit: coordinates of one predicate
    (queries included) whose last bits lie more than 38 binary places apart are snapped to a common grid.

    N < 2^31, T < 2^30, at most 2^30 queries.  CUDA tensors run the kernel (one synchronisation per call); CPU tensors a
    vectorised numpy walk with the same rule (Fractions where the double determinant is below its error bound)."""
    _check_points(points)
    if points.dtype != torch.float32:
        raise RuntimeError("points must be a float32 [N,3] tensor")
    _check_table("tets", points, tets)
    _check_table("tet_adjacency", points, tet_adjacency, tets.size(0))
    _check_queries(points, queries)
    if queries.dtype != torch.float32:
        raise RuntimeError("queries must be float32: the exact predicate takes float32 coordinates")
    shape = queries.shape[:-1]
    if start is not None and (not isinstance(start, torch.Tensor) or start.dtype not in _INDEX_DTYPES
                              or start.shape != shape or start.device != points.device):
        raise RuntimeError(f"start must be a uint32, int32 or int64 tensor of shape {list(shape)} on the device of points")
    n, nt, dev = points.size(0), tets.size(0), points.device
    max_hops = min(nt, 2 ** 20) if max_hops is None else int(max_hops)
    if max_hops < 0 or max_hops >= 2 ** 32:
        raise RuntimeError("max_hops must be in [0, 2^32)")
    p, q = points.detach().contiguous(), queries.detach().reshape(-1, 3).contiguous()
    s = None if start is None else start.reshape(-1)
    if q.size(0) == 0 or nt == 0:
        return TetLocation(torch.full(shape, -1, dtype=torch.int64, device=dev),
                           torch.zeros(shape, dtype=torch.int32, device=dev))
    if p.is_cuda:
        tet, hops, flags = _walk_hip(p, tets, tet_adjacency, q, s, max_hops)
        if any(flags.tolist()):                                      # the one synchronisation
            raise _fault_error(tet, s, n, nt, max_hops)
    else:
        tet, hops = _walk_host(p, tets, tet_adjacency, q, s, max_hops)
        if bool((tet < -1).any()):
            raise _fault_error(tet, s, n, nt, max_hops)
    return TetLocation(tet.reshape(shape), hops.reshape(shape))


# ---- interpolation ------------------------------------------------------------------------------------------------------

def _cross(a, b):
    return torch.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                        a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _field_torch(p, tets, v, q, tet):
    """(value [Q,C], weights [Q,4], gradient [Q,C,3], ok [Q], rows int64[Q,4]) in double, in the order of operations of
    rf_locate.hpp and before the NaN fill; plain torch, so autograd runs through it where the inputs ask for it"""
    n, nt, nq, dev = p.size(0), tets.size(0), q.size(0), p.device
    channels = v.size(1)
    if n == 0 or nt == 0:
        f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
        return (f64(nq, channels), f64(nq, 4), f64(nq, channels, 3), torch.zeros(nq, dtype=torch.bool, device=dev),
                torch.zeros((nq, 4), dtype=torch.int64, device=dev))
    ok = (tet >= 0) & (tet < nt)
    rows = _int64(tets)[tet.clamp(0, nt - 1)]
    ok = ok & ((rows >= 0) & (rows < n)).all(1)
    rows = rows.clamp(0, n - 1)
    corners = p.to(torch.float64)[rows]                                               # [Q,4,3]
    d1, d2, d3 = corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0], corners[:, 3] - corners[:, 0]
    x = q.to(torch.float64) - corners[:, 0]
    n1, n2, n3 = _cross(d2, d3), _cross(d3, d1), _cross(d1, d2)
    det = _dot(d1, n1)
    w1, w2, w3 = _dot(n1, x) / det, _dot(n2, x) / det, _dot(n3, x) / det
    w0 = 1.0 - ((w1 + w2) + w3)
    weights = torch.stack([w0, w1, w2, w3], 1)
    site_values = v.to(torch.float64)[rows]                                           # [Q,4,C]
    v0 = site_values[:, 0]
    e1, e2, e3 = site_values[:, 1] - v0, site_values[:, 2] - v0, site_values[:, 3] - v0
    gradient = ((e1[:, :, None] * n1[:, None, :] + e2[:, :, None] * n2[:, None, :]) + e3[:, :, None] * n3[:, None, :]) \
        / det[:, None, None]
    value = v0 + _dot(gradient, x[:, None, :])
    ok = ok & (det != 0.0) & torch.isfinite(weights).all(1) & torch.isfinite(gradient).reshape(nq, -1).all(1) \
        & torch.isfinite(value).all(1)
    return value, weights, gradient, ok, rows


def _forward_torch(p, tets, v, q, tet):
    value, weights, gradient, ok, _ = _field_torch(p, tets, v, q, tet)
    nan = float("nan")
    return (torch.where(ok[:, None], value, torch.full_like(value, nan)),
            torch.where(ok[:, None], weights, torch.full_like(weights, nan)),
            torch.where(ok[:, None, None], gradient, torch.full_like(gradient, nan)))


def _grad_parts_torch(p, tets, v, q, tet, g):
    """(parts f64[Q,4,3+C], grad_queries f64[Q,3], sites int64[Q,4] with N where the query adds nothing)"""
    n, nq, channels = p.size(0), q.size(0), v.size(1)
    _, weights, gradient, ok, rows = _field_torch(p, tets, v, q, tet)
    h = torch.zeros((nq, 3), dtype=torch.float64, device=p.device)
    for c in range(channels):
        h = h + g[:, c, None] * gradient[:, c]
    parts = torch.cat([-(weights[:, :, None] * h[:, None, :]), g[:, None, :] * weights[:, :, None]], 2)
    ok = ok & torch.isfinite(parts).reshape(nq, -1).all(1)
    parts = torch.where(ok[:, None, None], parts, torch.zeros_like(parts))
    return parts, torch.where(ok[:, None], h, torch.zeros_like(h)), torch.where(ok[:, None], rows, torch.full_like(rows, n))


def _grad_torch(p, tets, v, q, tet, g):
    n, channels = p.size(0), v.size(1)
    parts, grad_queries, sites = _grad_parts_torch(p, tets, v, q, tet, g)
    grad = torch.zeros((n + 1, 3 + channels), dtype=torch.float64, device=p.device)
    grad.index_add_(0, sites.reshape(-1), parts.reshape(-1, 3 + channels))
    return grad[:n, :3].contiguous(), grad[:n, 3:].contiguous(), grad_queries


def _forward_hip(p, tets, v, q, tet):
    n, nt, nq, channels, dev = p.size(0), tets.size(0), q.size(0), v.size(1), p.device
    tets = _kernel_table(tets)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    value, weights, gradient = f64(nq, channels), f64(nq, 4), f64(nq, channels, 3)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().rf_interpolate(_ptr(p), n, _ptr(tets), tets.element_size(), nt, _ptr(v), channels, _ptr(q),
                                              _ptr(tet), nq, _ptr(value), _ptr(weights), _ptr(gradient), _stream(dev)))
    return value, weights, gradient


def _incidence_sites(tets, tet, n):
    """int64[4Q]: the site of every corner of every query, N where the query has no tetrahedron or a corner out of range"""
    nt = tets.size(0)
    if nt == 0:
        return torch.full((4 * tet.numel(),), n, dtype=torch.int64, device=tet.device)
    rows = _int64(tets)[tet.clamp(0, nt - 1)]
    ok = (tet >= 0) & (tet < nt) & ((rows >= 0) & (rows < n)).all(1)
    return torch.where(ok[:, None], rows, torch.full_like(rows, n)).reshape(-1)


def _grad_hip(p, tets, v, q, tet, g):
    n, nt, nq, channels, dev = p.size(0), tets.size(0), q.size(0), v.size(1), p.device
    # the 4Q corners in order of site, ties in order of corner: the order in which a site's lane adds them
    sites, order = torch.sort(_incidence_sites(tets, tet, n), stable=True)
    runs = torch.searchsorted(sites, torch.arange(n + 1, dtype=torch.int64, device=dev)).contiguous()
    tets = _kernel_table(tets)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    parts, grad_points, grad_values, grad_queries = f64(nq, 4, 3 + channels), f64(n, 3), f64(n, channels), f64(nq, 3)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().rf_interpolate_grad(_ptr(p), n, _ptr(tets), tets.element_size(), nt, _ptr(v), channels,
                                                   _ptr(q), _ptr(tet), nq, _ptr(g), _ptr(order.contiguous()), _ptr(runs),
                                                   _ptr(parts), _ptr(grad_points), _ptr(grad_values), _ptr(grad_queries),
                                                   _stream(dev)))
    return grad_points, grad_values, grad_queries


def _check_field(points, tets, values, queries, tet):
    _check_points(points)
    _check_table("tets", points, tets)
    n = points.size(0)
    if (not isinstance(values, torch.Tensor) or values.dtype not in (torch.float32, torch.float64)
            or values.device != points.device or values.dim() not in (1, 2) or values.size(0) != n
            or (values.dim() == 2 and values.size(1) == 0)):
        raise RuntimeError(f"values must be a float32 or float64 [{n}] or [{n},C] tensor on the device of points")
    _check_queries(points, queries)
    if (not isinstance(tet, torch.Tensor) or tet.dtype != torch.int64 or tet.shape != queries.shape[:-1]
            or tet.device != points.device):
        raise RuntimeError(f"tet must be an int64 tensor of shape {list(queries.shape[:-1])} on the device of points")


def _backend(points, values, queries, backend):
    channels = values.size(1) if values.dim() == 2 else 1
    if backend is None and (values.dtype != torch.float32 or queries.dtype != torch.float32 or channels > _MAX_CHANNELS):
        backend = "torch"
    chosen = _choose_backend(backend, points, "points")
    if chosen == "hip":
        _choose_backend("hip", values, "values")
        _choose_backend("hip", queries, "queries")
        if channels > _MAX_CHANNELS:
            raise RuntimeError(f"the kernels serve at most {_MAX_CHANNELS} channels (backend='torch' restates them for more)")
    return chosen


def _flat(points, values, queries, tet):
    return (points.detach().contiguous(), values.detach().reshape(values.size(0), -1).contiguous(),
            queries.detach().reshape(-1, 3).contiguous(), tet.reshape(-1).contiguous())


def _grad_impl(backend, p, tets, v, q, tet, g):
    return (_grad_torch if backend == "torch" else _grad_hip)(p, tets, v, q, tet, g)


def interpolate_grad(points: torch.Tensor, tets: torch.Tensor, values: torch.Tensor, queries: torch.Tensor,
                     tet: torch.Tensor, grad_value: torch.Tensor, backend=None):
    """(grad_points f64[N,3], grad_values f64[N] or [N,C], grad_queries f64[...,3]): the gradients of
    sum grad_value * value, ``value`` being interpolate(points, tets, values, queries, tet).value.

    With g_c the field's gradient of channel c in the query's tetrahedron, w_i its weights and G_c the upstream:
    grad q = sum_c G_c g_c,  grad v_si,c = G_c w_i,  grad p_si = -w_i sum_c G_c g_c, in double.  A query that is NaN in
    the forward or whose terms are not finite adds nothing.  The kernels write the four corners' parts of every query
    once and one lane per site adds its own, in ascending order of corner entry: bit-reproducible, no atomics.
    ``backend`` as interpolate."""
    _check_field(points, tets, values, queries, tet)
    chosen = _backend(points, values, queries, backend)
    p, v, q, t = _flat(points, values, queries, tet)
    if (not isinstance(grad_value, torch.Tensor) or grad_value.device != points.device
            or not grad_value.dtype.is_floating_point or grad_value.numel() != q.size(0) * v.size(1)
            or grad_value.shape[:tet.dim()] != tet.shape):
        raise RuntimeError("grad_value must be a floating-point tensor of the shape of value on the device of points")
    g = grad_value.detach().to(torch.float64).reshape(q.size(0), v.size(1)).contiguous()
    gp, gv, gq = _grad_impl(chosen, p, tets, v, q, t, g)
    return gp, gv.reshape(values.shape), gq.reshape(queries.shape)


class _Interpolate(torch.autograd.Function):
    """(value [Q,C], weights [Q,4], gradient [Q,C,3]); weights and gradient are not differentiable"""

    @staticmethod
    def forward(ctx, points, values, queries, tets, tet, backend):
        p, v, q, t = _flat(points, values, queries, tet)
        ctx.save_for_backward(p, v, q, t, tets)
        ctx.backend = backend
        ctx.like = tuple((x.dtype, x.shape) for x in (points, values, queries))
        value, weights, gradient = (_forward_torch if backend == "torch" else _forward_hip)(p, tets, v, q, t)
        ctx.mark_non_differentiable(weights, gradient)
        return value, weights, gradient

    @staticmethod
    def backward(ctx, grad_value, _grad_weights, _grad_gradient):
        p, v, q, t, tets = ctx.saved_tensors
        gp, gv, gq = _grad_impl(ctx.backend, p, tets, v, q, t, grad_value.detach().to(torch.float64).contiguous())
        (pd, ps), (vd, vs), (qd, qs) = ctx.like
        return gp.to(pd).reshape(ps), gv.to(vd).reshape(vs), gq.to(qd).reshape(qs), None, None, None


def interpolate(points: torch.Tensor, tets: torch.Tensor, values: torch.Tensor, queries: torch.Tensor, tet: torch.Tensor,
                backend=None) -> FieldSamples:
    """The field of ``values`` (float32 or float64 [N] or [N,C], one row per site), interpolated linearly over every
    tetrahedron of ``tets`` -- the field isosurface extracts the level set of --, at ``queries`` ([...,3]), each in the
    row ``tet`` (int64[...], as locate_tets returns it) names.

    All arithmetic is in double, in the spelled order of csrc/rf_locate.hpp, with nothing fused:  d_i = p_si - p_s0,
    x = q - p_s0,  n_1 = d_2 x d_3, n_2 = d_3 x d_1, n_3 = d_1 x d_2,  det = d_1 . n_1,  w_i = (n_i . x) / det,
    w_0 = 1 - ((w_1 + w_2) + w_3),  g = sum_i (v_i - v_0) n_i / det,  value = v_0 + g . x.  ``weights`` (f64[...,4]) are
    not clamped (on a boundary they may be -1e-17) and carry any per-site attribute to the queries in torch
    ((weights[..., None] * attribute[tets[tet]]).sum(-2)).  ``gradient`` (f64[...,3] or [...,C,3]) is the field's spatial
    gradient, constant per tetrahedron.  ``weights`` and ``gradient`` are returned detached; ``value`` (f64[...] or
    [...,C]) is differentiable in ``values``, ``points`` and ``queries`` (interpolate_grad, returned in their dtypes).

    ``tet`` = -1 or outside [0, T), a corner index out of range, det == 0 or a result that is not finite give NaN in all
    three outputs of that query and add nothing backward.  Deterministic: two calls give the same bits.
    ``backend``: None (the kernels for float32 CUDA ``points``, ``values`` and ``queries`` and C <= 8, torch otherwise),
    "hip" or "torch"."""
    _check_field(points, tets, values, queries, tet)
    chosen = _backend(points, values, queries, backend)
    value, weights, gradient = _Interpolate.apply(points, values, queries, tets, tet, chosen)
    shape = tuple(tet.shape)
    if values.dim() == 1:
        return FieldSamples(value.reshape(shape), weights.reshape(shape + (4,)), gradient.reshape(shape + (3,)))
    return FieldSamples(value.reshape(shape + (values.size(1),)), weights.reshape(shape + (4,)),
                        gradient.reshape(shape + (values.size(1), 3)))
