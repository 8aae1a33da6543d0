"""The Voronoi cell of any point: the site nearest to it, by an exact greedy walk over the neighbour lists (DESIGN.md,
"Cell location").

  locate_cells   the cell of every query and the steps its walk took

csrc/rf_nearest.hpp states the definitions once (the closer predicate and its bound, the key, the step, the seeds, the
faults); the kernel of csrc/rf_nearest.hip behind the C-ABI of include/radfoam_hip_nearest.h, the host build of the tests
and the numpy restatement here share them to the letter.
"""
from __future__ import annotations

from fractions import Fraction
from typing import NamedTuple

import torch

from . import _lib
from .scene_ops import _ptr, _stream
from .segments import _choose_backend

_CLOSER_BOUND = 1.5e-15    # rf::nearest::kCloserBound
_MAX_SEEDS = 1024          # rf::nearest::kMaxSeeds
# rf::nearest::Fault
_BAD_START, _BAD_ROW, _BAD_ENTRY, _HOP_CAP = range(4)
_INDEX_DTYPES = (torch.uint32, torch.int32, torch.int64)
_OUT_OF_RANGE = 0xFFFFFFFF


class CellLocation(NamedTuple):
    cell: torch.Tensor   # int64[...]; a site with no site exactly nearer to the query, -1 for a query that is not finite
    hops: torch.Tensor   # int32[...]; the steps the walk took


def _fault_code(kind, site):
    return -2 - (kind + 8 * site)


def seed_sites(n, num_seeds):
    """int64[S]: the sites the walks are seeded from, floor(i N / S)"""
    return (torch.arange(num_seeds, dtype=torch.int64) * n) // max(num_seeds, 1)


# ---- the restatement ----------------------------------------------------------------------------------------------------

def _dist2(p, q):
    """D of rf_nearest.hpp for numpy float32 [...,3] arrays: double, in the spelled order"""
    import numpy as np
    d = p.astype(np.float64) - q.astype(np.float64)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def exact_closer(pa, pb, q):
    """the sign of |pa - q|^2 - |pb - q|^2 in Fractions of the float32 inputs"""
    x = [Fraction(float(v)) for v in q]
    da = sum((Fraction(float(v)) - x[k]) ** 2 for k, v in enumerate(pa))
    db = sum((Fraction(float(v)) - x[k]) ** 2 for k, v in enumerate(pb))
    return (da > db) - (da < db)


def _undecided(da, db):
    import numpy as np
    with np.errstate(invalid="ignore"):                                  # (padding: inf - inf)
        return np.logical_not(np.abs(da - db) > _CLOSER_BOUND * (da + db))


def _key_less(a, da, pa, b, db, pb, q):
    """rf::nearest::key_less for one pair"""
    if not _undecided(da, db):
        return bool(da < db)
    s = exact_closer(pa, pb, q)
    return s < 0 or (s == 0 and a < b)


def _smallest_key(index, d, p, q):
    """numpy int64[M]: per row of the padded candidates (index int64[M,W], -1 where there is none; d f64[M,W] with inf
    there; p f32[M,W,3]) the column of the smallest key, -1 for a row without candidates.  The smallest D is the smallest
    key unless another D lies within the bound of it; those rows are settled pair by pair, in list order."""
    import numpy as np
    first = d.argmin(1)
    rows = np.arange(len(d))
    dmin = d[rows, first]
    out = np.where(index[rows, first] >= 0, first, -1)
    rivals = (index >= 0) & _undecided(d, dmin[:, None])
    rivals[rows, first] = False
    for m in np.nonzero(rivals.any(1))[0]:
        best = -1
        for c in np.nonzero(index[m] >= 0)[0]:
            if not (c == first[m] or rivals[m, c]):
                continue
            if best < 0 or (index[m, c] != index[m, best]
                            and _key_less(index[m, c], d[m, c], p[m, c], index[m, best], d[m, best], p[m, best], q[m])):
                best = c
        out[m] = best
    return out


def _best_seeds_numpy(pts, sites, queries):
    """the site of the seed with the smallest key, per query"""
    import numpy as np
    out = np.zeros(len(queries), dtype=np.int64)
    staged = pts[sites]
    order = np.arange(len(sites), dtype=np.int64)
    for lo in range(0, len(queries), 1024):                              # bounds the [Q,S] table
        q = queries[lo:lo + 1024]
        d = _dist2(staged[None, :, :], q[:, None, :])
        p = np.broadcast_to(staged[None], (len(q),) + staged.shape)
        col = _smallest_key(np.broadcast_to(order[None], d.shape), d, p, q)
        out[lo:lo + 1024] = sites[col]
    return out


def _walk_numpy(pts, adj, offsets, queries, start, max_hops):
    """(cell int64[Q] with the fault codes of rf_nearest.hpp, hops int32[Q]) of numpy float32 pts [N,3] and finite queries
    [Q,3], int64 adj [E] / offsets [N+1] and int64 start [Q]: rf::nearest::walk, all queries at once"""
    import numpy as np
    n, ne, nq = len(pts), len(adj), len(queries)
    cell, hops = np.full(nq, -1, dtype=np.int64), np.zeros(nq, dtype=np.int32)
    bad = (start < 0) | (start >= n)
    cell[bad] = _fault_code(_BAD_START, 0)
    active = np.nonzero(~bad)[0]
    cur, taken = start[active].astype(np.int64), np.zeros(len(active), dtype=np.int64)

    def settle(which, result):
        nonlocal active, cur, taken
        cell[active[which]], hops[active[which]] = result, taken[which]
        active, cur, taken = active[~which], cur[~which], taken[~which]

    while len(active):
        begin, end = offsets[cur], offsets[cur + 1]
        broken = (begin < 0) | (begin > end) | (end > ne)
        if broken.any():
            settle(broken, _fault_code(_BAD_ROW, cur[broken]))
            continue
        degree = end - begin
        width = max(int(degree.max()), 1)
        cols = np.arange(width, dtype=np.int64)[None, :]
        have = cols < degree[:, None]
        slot = np.where(have, begin[:, None] + cols, 0)
        entry = np.where(have, adj[slot], -1) if ne else np.full(slot.shape, -1, dtype=np.int64)
        outside = (have & ((entry < 0) | (entry >= n))).any(1)
        if outside.any():
            settle(outside, _fault_code(_BAD_ENTRY, cur[outside]))
            continue
        q = queries[active]
        p = pts[entry.clip(0, n - 1)]
        d = np.where(have, _dist2(p, q[:, None, :]), np.inf)
        col = _smallest_key(entry, d, p, q)
        rows = np.arange(len(active))
        best = np.where(col >= 0, entry[rows, col.clip(0)], -1)
        dbest, pbest = d[rows, col.clip(0)], p[rows, col.clip(0)]
        ps = pts[cur]
        ds = _dist2(ps, q)
        goes = (best >= 0) & (best != cur) & ~_undecided(dbest, ds) & (dbest < ds)
        for m in np.nonzero((best >= 0) & (best != cur) & _undecided(dbest, ds))[0]:
            goes[m] = _key_less(best[m], dbest[m], pbest[m], cur[m], ds[m], ps[m], q[m])
        if (~goes).any():
            settle(~goes, cur[~goes])
            continue
        capped = taken >= max_hops
        if capped.any():
            settle(capped, _fault_code(_HOP_CAP, cur[capped]))
            continue
        cur, taken = best, taken + 1
    return cell, hops


def _locate_host(p, adj, offsets, q, start, num_seeds, max_hops):
    import numpy as np
    pts, queries = p.numpy(), q.numpy()
    n, nq = len(pts), len(queries)
    cell, hops = np.full(nq, -1, dtype=np.int64), np.zeros(nq, dtype=np.int32)
    finite = np.isfinite(queries).all(1)
    if start is not None:
        s = start.to(torch.int64).numpy()[finite]
    elif num_seeds:
        s = _best_seeds_numpy(pts, seed_sites(n, num_seeds).numpy(), queries[finite])
    else:
        s = np.zeros(int(finite.sum()), dtype=np.int64)
    cell[finite], hops[finite] = _walk_numpy(pts, adj.to(torch.int64).numpy(), offsets.to(torch.int64).numpy(),
                                             queries[finite], s, max_hops)
    return torch.from_numpy(cell), torch.from_numpy(hops)


# ---- the kernel -------------------------------------------------------------------------------------------------------

def _words(t):
    """the list as the 4-byte words the kernel reads (a contiguous int32-typed tensor, at the tensor's own address where
    it has these words already); an int64 value outside [0, 2^32) becomes 0xFFFFFFFF, which is out of every range"""
    if t.dtype == torch.uint32:
        return t.contiguous().view(torch.int32)
    if t.dtype == torch.int32:
        return t.contiguous()
    t = torch.where((t < 0) | (t > _OUT_OF_RANGE), torch.full_like(t, _OUT_OF_RANGE), t)
    return (t - ((t >> 31) << 32)).to(torch.int32).contiguous()          # the low word, as int32


def _locate_hip(p, adj, offsets, q, start, num_seeds, max_hops):
    """(cell, hops, flags int32[2]) on the device; nothing synchronises"""
    n, ne, nq, dev = p.size(0), adj.numel(), q.size(0), p.device
    adj, offsets = _words(adj), _words(offsets)
    s = None if start is None else start.to(torch.int64).contiguous()
    cell = torch.empty(nq, dtype=torch.int64, device=dev)
    hops = torch.empty(nq, dtype=torch.int32, device=dev)
    flags = torch.zeros(2, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().rf_locate_cells(_ptr(p), n, _ptr(adj) if ne else None, _ptr(offsets), ne, _ptr(q),
                                               None if s is None else _ptr(s), num_seeds, nq, max_hops, _ptr(cell),
                                               _ptr(hops), _ptr(flags), _stream(dev)))
    return cell, hops, flags


def _fault_error(cell, start, n, ne, max_hops):
    """the RuntimeError of the first faulted query (found on this path only)"""
    k = int(torch.nonzero(cell < -1)[0])
    code = -2 - int(cell[k])
    kind, site = code & 7, code >> 3
    what = {_BAD_START: f"its start {0 if start is None else int(start[k])} is outside [0, {n})",
            _BAD_ROW: f"the row of site {site} has bounds in point_adjacency_offsets that run backwards or past {ne}",
            _BAD_ENTRY: f"the row of site {site} has an entry outside [0, {n})",
            _HOP_CAP: f"its walk would take more than max_hops = {max_hops} steps (at site {site}): max_hops is too "
                      "small, or the coordinates span more than the exact predicate's 38 binary places"}[kind]
    return RuntimeError(f"locate_cells: query {k}: {what}")


def locate_cells(points: torch.Tensor, adj: torch.Tensor, offsets: torch.Tensor, queries: torch.Tensor, start=None,
                 seeds=None, max_hops=None, backend=None) -> CellLocation:
    """The Voronoi cell of every query (float32 [...,3]): a site of ``points`` (float32 [N,3], N >= 1) with no site exactly
    nearer to the query, by a greedy walk over the neighbour lists ``adj`` [E] / ``offsets`` [N+1] (uint32, int32 or int64,
    as Triangulation.point_adjacency() / point_adjacency_offsets() return them and cell_geometry takes them: row i is
    adj[offsets[i]:offsets[i+1]]).

    Sites are ordered by the key (exact squared distance to the query, index).  At a site the walk scans its row in list
    order for the entry with the smallest key and goes there if that key is below the site's own; otherwise the site is
    the answer.  ``cell`` (int64[...]) is that site, ``hops`` (int32[...]) the steps taken.  A query with a coordinate that
    is not finite gets -1 and 0 hops; every finite query has a cell.  The comparison is exact for float32 inputs: the
    squared distances in double where they differ by more than their error bound, 384-bit integers below it
    (csrc/rf_nearest.hpp), with the documented limit of that path: coordinates of one predicate (two sites and the query)
    whose last bits lie more than 38 binary places apart are snapped to a common grid.

    ``start`` (uint32, int32 or int64 [...]): the site every walk starts at, in [0, N).  Without it the walk is seeded:
    of the S = min(N, ``seeds`` or 1024) sites floor(i N / S) the one with the smallest key is the start (``seeds`` at
    most 1024; Triangulation keeps its points kd-ordered, so strided seeds are spread in space; for unordered points the
    result is as correct and the walk longer).  ``seeds=0`` starts every walk at site 0.

    Guaranteed on any lists: a returned cell has no entry of its own row with a smaller key.  On the neighbour lists of a
    Delaunay triangulation of ``points`` it is a global nearest site: the nearest site where that is unique, whatever the
    start; one of them where several tie exactly, and which one depends on the start.  With equal starts the result is the
    same on every backend, bit for bit, ``hops`` included.  The key falls at every step, so the walk ends; ``max_hops``
    (default min(N, 2^20)) caps it all the same, and a walk that would take more steps raises RuntimeError naming the
    first such query.  So do, naming the first offender: a start outside [0, N), a row whose bounds in ``offsets`` run
    backwards or past E, and a list entry outside [0, N).

    N < 2^31, at most 2^30 queries.  ``backend``: None (the kernel for CUDA tensors, one synchronisation per call; a
    vectorised numpy walk with the same rule for CPU tensors), "hip" or "torch"."""
    if (not isinstance(points, torch.Tensor) or points.dim() != 2 or points.size(-1) != 3 or points.dtype != torch.float32):
        raise RuntimeError("points must be a float32 [N,3] tensor")
    n, dev = points.size(0), points.device
    if n == 0 or n >= 2 ** 31:
        raise RuntimeError("locate_cells takes between 1 and 2^31 - 1 points")
    for name, t in (("adj", adj), ("offsets", offsets)):
        if not isinstance(t, torch.Tensor) or t.dtype not in _INDEX_DTYPES or t.dim() != 1 or t.device != dev:
            raise RuntimeError(f"{name} must be a one-dimensional uint32, int32 or int64 tensor on the device of points")
    if offsets.numel() != n + 1:
        raise RuntimeError("expected adj [E] and offsets [N+1]")
    if adj.numel() >= 2 ** 32:
        raise RuntimeError("2^32 adjacency entries or more")
    if (not isinstance(queries, torch.Tensor) or queries.dim() < 1 or queries.size(-1) != 3
            or queries.dtype != torch.float32 or queries.device != dev):
        raise RuntimeError("queries must be a float32 [...,3] tensor on the device of points: the exact predicate takes "
                           "float32 coordinates")
    if queries.numel() // 3 > 2 ** 30:
        raise RuntimeError("more than 2^30 queries")
    shape = queries.shape[:-1]
    if start is not None and (not isinstance(start, torch.Tensor) or start.dtype not in _INDEX_DTYPES
                              or start.shape != shape or start.device != dev):
        raise RuntimeError(f"start must be a uint32, int32 or int64 tensor of shape {list(shape)} on the device of points")
    seeds = _MAX_SEEDS if seeds is None else int(seeds)
    if seeds < 0 or seeds > _MAX_SEEDS:
        raise RuntimeError(f"seeds must be in [0, {_MAX_SEEDS}]")
    num_seeds = 0 if start is not None else min(n, seeds)
    max_hops = min(n, 2 ** 20) if max_hops is None else int(max_hops)
    if max_hops < 0 or max_hops >= 2 ** 32:
        raise RuntimeError("max_hops must be in [0, 2^32)")
    chosen = _choose_backend(backend, points, "points")
    if chosen == "hip":
        _choose_backend("hip", queries, "queries")
    p, q = points.detach().contiguous(), queries.detach().reshape(-1, 3).contiguous()
    s = None if start is None else start.reshape(-1)
    if s is not None and s.dtype == torch.uint32:
        s = s.view(torch.int32).to(torch.int64) & _OUT_OF_RANGE
    if q.size(0) == 0:
        return CellLocation(torch.full(shape, -1, dtype=torch.int64, device=dev),
                            torch.zeros(shape, dtype=torch.int32, device=dev))
    ne = adj.numel()
    if chosen == "hip":
        cell, hops, flags = _locate_hip(p, adj, offsets, q, s, num_seeds, max_hops)
        if any(flags.tolist()):                                      # the one synchronisation
            raise _fault_error(cell, s, n, ne, max_hops)
    else:
        cell, hops = _locate_host(p.cpu(), _as_int64(adj).cpu(), _as_int64(offsets).cpu(), q.cpu(),
                                  None if s is None else s.cpu(), num_seeds, max_hops)
        cell, hops = cell.to(dev), hops.to(dev)
        if bool((cell < -1).any()):
            raise _fault_error(cell, s, n, ne, max_hops)
    return CellLocation(cell.reshape(shape), hops.reshape(shape))


def _as_int64(t):
    """the list's values as int64: uint32 words above 2^31 stay positive"""
    if t.dtype == torch.uint32:
        return t.view(torch.int32).to(torch.int64) & _OUT_OF_RANGE
    return t.to(torch.int64)
