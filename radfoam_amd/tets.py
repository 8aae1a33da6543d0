"""The Delaunay tetrahedra read back off the neighbour lists ("Tetrahedra from the neighbour lists").

  delaunay_tets   (points, point_adjacency, point_adjacency_offsets) -> DelaunayTets

The Voronoi cell of a site is the intersection of the half-spaces of its Delaunay neighbours alone, so the star of a
site in the triangulation of the site and its neighbours is its star in the full triangulation.  On the device every row
of the lists is inserted into a fresh star with exact predicates (csrc/rf_star.hpp) and the tetrahedra are read off the
link: csrc/rf_tets.hip behind the C-ABI of include/radfoam_hip_tets.h; csrc/rf_tets.hpp states the definitions.  The
scans (torch.cumsum) and the sort of the faces for ``tet_adjacency`` are torch on the device.  CPU tensors go through
Qhull and are compared with the given lists; that path makes no claim on speed.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _lib
from .scene_ops import _ptr, _stream
from .triangulation import TriangulationFailedError

# rf::tets::Code (csrc/rf_tets.hpp)
_OK, _NEED_BIG, _NEED_HUGE, _OK_BIG, _OK_HUGE = 0, 1, 2, 4, 5
_MALFORMED = {8: "its offsets are not monotone or do not end at the length of point_adjacency",
              9: "it names an index outside [0, N)", 10: "it names itself", 11: "it names a site twice",
              12: "it has more than 4095 neighbours"}
_FAILED = {16: "without a non-coplanar start", 17: "inconsistent", 18: "with a duplicate point",
           19: "with an entry that is not a Delaunay neighbour"}


class DelaunayTets(NamedTuple):
    tets: torch.Tensor                     # uint32[T,4]; smallest site first, positive orientation, rows ascending
    vert_to_tet: torch.Tensor              # uint32[N]; the smallest row with the site
    tet_adjacency: Optional[torch.Tensor]  # uint32[T,4]; 4 t' + j' across the face opposite corner j, 0xFFFFFFFF on the hull
    hull_faces: int


def _words(name, t, dev):
    """the list as int32 words on the device of points; a value out of range stays out of range"""
    if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.device != dev:
        raise RuntimeError(f"{name} must be a 1-d tensor on the device of points")
    if t.dtype == torch.uint32:
        return t.contiguous().view(torch.int32)
    if t.dtype == torch.int32:
        return t.contiguous()
    if t.dtype == torch.int64:
        return t.clamp(-1, 2 ** 31 - 1).to(torch.int32).contiguous()
    raise RuntimeError("point_adjacency and point_adjacency_offsets must have uint32, int32 or int64 dtype")


def _u32(t):
    return t.view(torch.uint32)


def _malformed(row, kind):
    return RuntimeError(f"delaunay_tets: row {row} of the neighbour lists is malformed: {_MALFORMED[kind]}")


def _failed(counts, extra=""):
    parts = ", ".join(f"{counts[k]} {_FAILED[k]}" for k in sorted(_FAILED) if counts.get(k))
    return TriangulationFailedError("delaunay_tets: the neighbour lists are not those of a Delaunay triangulation of the "
                                    f"points ({sum(counts.values())} stars failed: {parts or 'none'}{extra})")


# ---- the device -------------------------------------------------------------------------------------------------------

stage_hook = None   # scripts/gpu_tets_time.py: called with the name of every stage of a call as it has been enqueued


def _mark(name):
    if stage_hook is not None:
        stage_hook(name)


def _large_rows(code, kind):
    return torch.nonzero(code == kind).flatten().contiguous()


def _tets_hip(p, adj, off, adjacency):
    n, e, dev = p.size(0), adj.numel(), p.device
    lib = _lib.load()
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    code = torch.empty(n, dtype=torch.uint8, device=dev)
    entries, owned, ghosts = i32(n), i32(n), i32(n)
    owned_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    entries_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    finite = torch.isfinite(p).all().to(torch.int64).reshape(1)
    lists = (_ptr(p), n, _ptr(adj), e, _ptr(off))
    _mark("start")
    with torch.cuda.device(dev):
        _lib.check(lib.rf_tets_count(*lists, _ptr(code), _ptr(entries), _ptr(owned), _ptr(ghosts), _stream(dev)))
    _mark("count")

    def scan():
        """the two scans; (codes by kind, T, F, ghosts, points finite) in one read-back"""
        torch.cumsum(owned, 0, dtype=torch.int64, out=owned_off[1:])
        torch.cumsum(entries, 0, dtype=torch.int64, out=entries_off[1:])
        kinds = torch.bincount(code, minlength=32)[:32].to(torch.int64)
        got = torch.cat([kinds, owned_off[-1:], entries_off[-1:], ghosts.sum(dtype=torch.int64).reshape(1), finite]).tolist()
        return got[:32], got[32], got[33], got[34], got[35]

    kinds, nt, nf, ng, ok = scan()
    _mark("scans and read-back")
    workspace = {}
    for instance, need in ((1, _NEED_BIG), (2, _NEED_HUGE)):   # rare: rows of more than 63 neighbours
        if ok and kinds[need]:
            rows = _large_rows(code, need)
            ws = workspace[instance] = torch.empty(int(lib.rf_tets_large_workspace_bytes(instance)), dtype=torch.uint8,
                                                   device=dev)
            with torch.cuda.device(dev):
                _lib.check(lib.rf_tets_count_large(instance, *lists, _ptr(rows), rows.numel(), _ptr(code), _ptr(entries),
                                                   _ptr(owned), _ptr(ghosts), _ptr(ws), ws.numel(), _stream(dev)))
            kinds, nt, nf, ng, ok = scan()
            _mark("count, larger instance %d" % instance)
    if not ok:
        raise RuntimeError("delaunay_tets: points contain non-finite values")
    if any(kinds[k] for k in _MALFORMED):
        row = int(torch.nonzero((code >= 8) & (code < 16))[0])
        raise _malformed(row, int(code[row]))
    if any(kinds[k] for k in _FAILED) or kinds[_NEED_BIG] or kinds[_NEED_HUGE]:
        raise _failed({k: kinds[k] for k in _FAILED})
    if nt > 2 ** 30:
        raise RuntimeError("delaunay_tets: more than 2^30 tetrahedra")
    if nf != 4 * nt or ng % 3:
        raise _failed({}, f"; {nf} star triangles for {nt} tetrahedra, {ng} hull facets at the sites")

    tets, star_entries, faults = i32(nt, 4), i32(nf, 3), i32(n)
    ticks = torch.zeros(4 * nt, dtype=torch.uint8, device=dev)
    missing, vert_to_tet = i32(n), i32(n)
    totals = (_ptr(owned_off), _ptr(entries_off), nt, nf, _ptr(tets), _ptr(star_entries), _ptr(faults))
    with torch.cuda.device(dev):
        _lib.check(lib.rf_tets_emit(*lists, _ptr(code), *totals, _stream(dev)))
        _mark("emit")
        for instance, kind in ((1, _OK_BIG), (2, _OK_HUGE)):
            if kinds[kind]:
                rows, ws = _large_rows(code, kind), workspace[instance]
                _lib.check(lib.rf_tets_emit_large(instance, *lists, _ptr(rows), rows.numel(), _ptr(code), *totals, _ptr(ws),
                                                  ws.numel(), _stream(dev)))
                _mark("emit, larger instance %d" % instance)
        _lib.check(lib.rf_tets_match(n, _ptr(star_entries), _ptr(entries_off), nf, _ptr(tets), _ptr(owned_off), nt,
                                     _ptr(ticks), _ptr(missing), _ptr(vert_to_tet), _stream(dev)))
    _mark("match")
    bad_rows, lost, ticked = torch.stack([(faults != 0).sum(), (missing != 0).sum(),
                                          ticks.sum(dtype=torch.int64)]).tolist()   # the second read-back
    _mark("sums and read-back")
    if bad_rows or lost or ticked != 4 * nt:
        raise _failed({}, f"; {bad_rows} sites with a flat or repeated tetrahedron, {lost} sites with a star triangle their "
                          f"owner does not hold, {4 * nt - ticked} of {4 * nt} corners unconfirmed")
    tet_adjacency = None
    if adjacency:
        tet_adjacency = _adjacency_hip(lib, tets, n, ng // 3)
    return DelaunayTets(_u32(tets), _u32(vert_to_tet), tet_adjacency, ng // 3)


_FACE_CORNERS = [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]]


def _face_order(faces, n):
    """int64[4T]: the faces (ascending triples, int64[4T,3]) in ascending lexicographic order, ties in order of index"""
    if n <= 2 ** 21:
        key = (faces[:, 0] << 42) | (faces[:, 1] << 21) | faces[:, 2]
        return torch.sort(key, stable=True).indices
    order = torch.sort(faces[:, 2], stable=True).indices
    for col in (1, 0):
        order = order[torch.sort(faces[order, col], stable=True).indices]
    return order


def _adjacency_hip(lib, tets, n, hull_faces):
    nt, dev = tets.size(0), tets.device
    out = torch.empty((nt, 4), dtype=torch.int32, device=dev)
    if nt == 0:
        return _u32(out)
    faces = tets.to(torch.int64)[:, _FACE_CORNERS].sort(dim=2).values.reshape(-1, 3)
    order = _face_order(faces, n).contiguous()
    _mark("faces sorted")
    single = torch.empty(4 * nt, dtype=torch.uint8, device=dev)
    fault = torch.empty(4 * nt, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.rf_tets_pair_faces(_ptr(tets), nt, _ptr(order), _ptr(out), _ptr(single), _ptr(fault), _stream(dev)))
    _mark("faces paired")
    singles, faults = torch.stack([single.sum(dtype=torch.int64), fault.sum(dtype=torch.int64)]).tolist()
    _mark("face sums and read-back")
    if faults or singles != hull_faces:
        raise _failed({}, f"; {faults} faces shared by more than two tetrahedra, {singles} unpaired faces for "
                          f"{hull_faces} hull facets")
    return _u32(out)


# ---- the host ---------------------------------------------------------------------------------------------------------

def _exact_sign(q):
    """the sign of det[q1 - q0; q2 - q0; q3 - q0] of four float32 points, in integers"""
    from fractions import Fraction
    f = [[Fraction(float(x)) for x in row] for row in q]
    a, b, c = ([f[k][d] - f[0][d] for d in range(3)] for k in (1, 2, 3))
    det = (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]))
    return (det > 0) - (det < 0)


def canonical_rows(points, simplices):
    """numpy int64[T,4]: every simplex with its sites ascending and the last two swapped where that makes
    det[p1 - p0; p2 - p0; p3 - p0] positive, rows in ascending lexicographic order of the sorted sets.  The sign is the
    double determinant's where it exceeds its forward error bound -- a term of the expansion carries three roundings of
    its differences' and two of its products', the sum five more: 10 * 2^-53 = 1.1e-15 of the sum of the absolute
    terms; 4e-15 leaves a factor of three -- and exact (Fractions) below.  A flat simplex raises
    TriangulationFailedError."""
    import numpy as np
    rows = np.sort(np.asarray(simplices, dtype=np.int64).reshape(-1, 4), axis=1)
    rows = rows[np.lexsort(rows.T[::-1])]
    q = np.asarray(points, dtype=np.float32).astype(np.float64)[rows]
    a, b, c = q[:, 1] - q[:, 0], q[:, 2] - q[:, 0], q[:, 3] - q[:, 0]
    terms = np.stack([a[:, 0] * b[:, 1] * c[:, 2], -a[:, 0] * b[:, 2] * c[:, 1], -a[:, 1] * b[:, 0] * c[:, 2],
                      a[:, 1] * b[:, 2] * c[:, 0], a[:, 2] * b[:, 0] * c[:, 1], -a[:, 2] * b[:, 1] * c[:, 0]], 1)
    det, perm = terms.sum(1), np.abs(terms).sum(1)
    sign = np.sign(det).astype(np.int64)
    for t in np.nonzero(~(np.abs(det) > 4.0e-15 * perm))[0]:
        sign[t] = _exact_sign(np.asarray(points, dtype=np.float32)[rows[t]])
    if (sign == 0).any():
        raise TriangulationFailedError(f"delaunay_tets: {int((sign == 0).sum())} flat tetrahedra")
    swap = sign < 0
    rows[swap, 2], rows[swap, 3] = rows[swap, 3].copy(), rows[swap, 2].copy()
    return rows


def mesh_tables(rows, n):
    """(vert_to_tet int64[n] with -1 for none, tet_adjacency int64[T,4] with -1 on the hull, hull_faces) of numpy rows"""
    import numpy as np
    nt = rows.shape[0]
    vert_to_tet = np.full(n, nt, dtype=np.int64)
    np.minimum.at(vert_to_tet, rows.reshape(-1), np.repeat(np.arange(nt), 4))
    vert_to_tet[vert_to_tet == nt] = -1
    faces = np.sort(rows[:, _FACE_CORNERS], axis=2).reshape(-1, 3)
    order = np.lexsort(faces.T[::-1])
    s = faces[order]
    same = (s[1:] == s[:-1]).all(1)
    if (same[1:] & same[:-1]).any():
        raise TriangulationFailedError("delaunay_tets: a face is shared by more than two tetrahedra")
    adjacency = np.full(4 * nt, -1, dtype=np.int64)
    first = np.nonzero(same)[0]
    adjacency[order[first]] = order[first + 1]
    adjacency[order[first + 1]] = order[first]
    return vert_to_tet, adjacency.reshape(nt, 4), int(4 * nt - 2 * len(first))


def _check_lists_host(adj, off, n):
    import numpy as np
    e = adj.shape[0]
    for i in range(n):
        a, b = int(off[i]), int(off[i + 1])
        if a > b or b > e or a < 0 or (i == 0 and a != 0) or (i + 1 == n and b != e):
            raise _malformed(i, 8)
        row = adj[a:b]
        if b - a > 4095:
            raise _malformed(i, 12)
        if ((row < 0) | (row >= n)).any():
            raise _malformed(i, 9)
        if (row == i).any():
            raise _malformed(i, 10)
        if len(np.unique(row)) != len(row):
            raise _malformed(i, 11)


def _tets_host(p, adj, off, adjacency):
    import numpy as np
    from scipy.spatial import Delaunay
    from scipy.spatial import QhullError
    n = p.size(0)
    pts = p.numpy()
    a64, o64 = adj.to(torch.int64).numpy(), off.to(torch.int64).numpy()
    if not np.isfinite(pts).all():
        raise RuntimeError("delaunay_tets: points contain non-finite values")
    _check_lists_host(a64, o64, n)
    try:
        mesh = Delaunay(pts.astype(np.float64))
    except (QhullError, ValueError) as exc:
        raise TriangulationFailedError(f"delaunay_tets: {exc}") from exc
    rows = canonical_rows(pts, mesh.simplices)
    pairs = rows[:, [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]].reshape(-1, 2)
    pairs = np.concatenate([pairs, pairs[:, ::-1]])
    mine = np.unique(pairs[:, 0] * n + pairs[:, 1])
    given = np.sort(np.repeat(np.arange(n, dtype=np.int64), np.diff(o64)) * n + a64)
    if not np.array_equal(mine, given):
        extra, lost = len(np.setdiff1d(given, mine)), len(np.setdiff1d(mine, given))
        raise _failed({}, f"; {extra} list entries are not Delaunay edges, {lost} Delaunay edges are not in the lists")
    vert_to_tet, tet_adjacency, hull_faces = mesh_tables(rows, n)
    as_u32 = lambda x: torch.from_numpy(np.ascontiguousarray(x.astype(np.int64).astype(np.uint32)))
    return DelaunayTets(as_u32(rows), as_u32(vert_to_tet), as_u32(tet_adjacency) if adjacency else None, hull_faces)


def delaunay_tets(points: torch.Tensor, point_adjacency: torch.Tensor, point_adjacency_offsets: torch.Tensor,
                  adjacency: bool = False) -> DelaunayTets:
    """The tetrahedra of the Delaunay triangulation whose neighbour lists are ``point_adjacency`` /
    ``point_adjacency_offsets`` (uint32, int32 or int64, as Triangulation gives them) over ``points`` (float32 [N,3]).

    ``tets`` uint32[T,4]: the four sites of every tetrahedron, the smallest first, then the others ascending with the
    last two swapped where needed so that det[p1 - p0; p2 - p0; p3 - p0] > 0 (exact sign; the orientation isosurface
    calls positive); rows in ascending lexicographic order of their sorted site sets (the order of the reference's
    ``tets()``).  ``vert_to_tet`` uint32[N]: the smallest row with the site.  ``tet_adjacency`` (``adjacency=True``)
    uint32[T,4]: 4 t' + j' for the tetrahedron t' across the face opposite corner j, j' that face's corner in t', and
    0xFFFFFFFF on the hull; ``hull_faces`` the number of hull facets.  Bit-reproducible.

    Raises RuntimeError naming the first malformed row (offsets not monotone or not ending at the length of the
    adjacency, an index outside [0, N), a row naming itself or a site twice, more than 4095 neighbours) and
    TriangulationFailedError when the lists are not those of the Delaunay triangulation of the points (stale lists,
    lists of cospherical points): every returned row is confirmed by the stars of all four of its sites.
    N < 2^31, T <= 2^30.  CUDA tensors run the kernels; CPU tensors go through Qhull and are compared with the lists."""
    if (not isinstance(points, torch.Tensor) or points.dim() != 2 or points.size(-1) != 3
            or points.dtype != torch.float32):
        raise RuntimeError("points must be a float32 [N,3] tensor")
    n, dev = points.size(0), points.device
    if n >= 2 ** 31:
        raise RuntimeError("more than 2^31 points")
    if isinstance(point_adjacency, torch.Tensor) and point_adjacency.numel() >= 2 ** 31:
        raise RuntimeError("more than 2^31 adjacency entries")
    adj = _words("point_adjacency", point_adjacency, dev)
    off = _words("point_adjacency_offsets", point_adjacency_offsets, dev)
    if off.numel() != n + 1:
        raise RuntimeError(f"point_adjacency_offsets must have {n + 1} entries")
    p = points.detach().contiguous()
    if n == 0:
        empty = torch.zeros((0, 4), dtype=torch.int32, device=dev)
        return DelaunayTets(_u32(empty), _u32(empty[:, 0].clone()), _u32(empty.clone()) if adjacency else None, 0)
    if p.is_cuda:
        return _tets_hip(p, adj, off, bool(adjacency))
    return _tets_host(p, adj, off, bool(adjacency))
