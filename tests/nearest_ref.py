"""Reference for radfoam.locate_cells (helper, no GPU): the clouds with Qhull's neighbour lists (tests/tets_ref.py), the
queries the CPU and GPU tests share, the exact nearest sites by brute force in Fractions of the float32 inputs, the stale
and the malformed lists."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from tests import tets_ref as T

KINDS = ("uniform", "clustered", "offset", "scaled")
SIZES = (64, 400, 3000)
CLOUDS = [(kind, n) for kind in KINDS for n in SIZES] + [("hub", 301)]
# (kind, n) -> the cloud's seed where the default one does not serve: scaled / 64 has 6 exact two-way ties with seed 4
_SEED = {("scaled", 64): 5}
_CLOUD, _QUERIES, _NEAREST = {}, {}, {}


def hub(seed=5):
    """one centre site (index 0) and 300 sites at radius 1 +- 10 %: the centre's row has about 300 entries"""
    rng = np.random.default_rng(seed)
    shell = rng.normal(size=(300, 3))
    shell *= rng.uniform(0.9, 1.1, size=(300, 1)) / np.linalg.norm(shell, axis=1, keepdims=True)
    return np.concatenate([np.zeros((1, 3)), shell]).astype(np.float32)


def cloud(kind, n) -> dict:
    """dict(points f32[N,3], adjacency uint32[E], offsets uint32[N+1], simplices, ...) of a named cloud through Qhull
    (tets_ref.reference), computed once and shared; callers leave it unchanged"""
    if (kind, n) not in _CLOUD:
        if kind == "hub":
            pts = hub(*([_SEED[(kind, n)]] if (kind, n) in _SEED else []))
        else:
            pts = T.KINDS[kind](n, *([_SEED[(kind, n)]] if (kind, n) in _SEED else []))
        _CLOUD[(kind, n)] = T.reference(pts)
    return _CLOUD[(kind, n)]


def row(m, i):
    return m["adjacency"][int(m["offsets"][i]):int(m["offsets"][i + 1])].astype(np.int64)


# ---- exact --------------------------------------------------------------------------------------------------------------

def _frac(p):
    return [Fraction(float(x)) for x in p]


def exact_dist2(p, q):
    return sum((a - b) ** 2 for a, b in zip(_frac(p), _frac(q)))


def nearest_sites(points, q, among=None):
    """the sites (ascending) at the smallest exact squared distance to the finite q, by brute force over all sites (or
    over ``among``): the double distances first, Fractions for those within 1e-12 relative of the smallest"""
    idx = np.arange(len(points)) if among is None else np.asarray(among, dtype=np.int64)
    d = ((points[idx].astype(np.float64) - q.astype(np.float64)) ** 2).sum(1)
    close = idx[d <= d.min() * (1 + 1e-12) + 1e-300]
    exact = [exact_dist2(points[s], q) for s in close]
    least = min(exact)
    return np.array(sorted(int(s) for s, e in zip(close, exact) if e == least), dtype=np.int64)


def nearest_of(kind, n):
    """per query of queries(kind, n): the exact nearest sites, None for a query that is not finite; computed once"""
    if (kind, n) not in _NEAREST:
        pts, q = cloud(kind, n)["points"], queries(kind, n)["q"]
        _NEAREST[(kind, n)] = [nearest_sites(pts, x) if np.isfinite(x).all() else None for x in q]
    return _NEAREST[(kind, n)]


def check_nearest(kind, n, cell):
    """every cell is a nearest site by the exact reference (the one where it is unique), -1 exactly where the query is
    not finite; returns the number of mismatches, which the tests hold at zero"""
    wrong = 0
    for k, want in enumerate(nearest_of(kind, n)):
        wrong += (cell[k] != -1) if want is None else (int(cell[k]) not in want.tolist())
    return int(wrong)


def check_local_minimum(points, adj, offsets, q, cell):
    """no entry of the returned cell's row has a smaller exact key (squared distance, index)"""
    for k in range(len(q)):
        if cell[k] < 0:
            continue
        s = int(cell[k])
        own = (exact_dist2(points[s], q[k]), s)
        entries = np.asarray(adj[int(offsets[s]):int(offsets[s + 1])]).astype(np.int64)
        d = ((points[entries].astype(np.float64) - q[k].astype(np.float64)) ** 2).sum(1)
        mine = float(((points[s].astype(np.float64) - q[k].astype(np.float64)) ** 2).sum())
        for e in entries[d <= mine * (1 + 1e-12) + 1e-300]:
            assert (exact_dist2(points[int(e)], q[k]), int(e)) >= own, (k, s, int(e))


# ---- the queries --------------------------------------------------------------------------------------------------------

def _circumcentre(p):
    a = p[1:] - p[0]
    return p[0] + np.linalg.solve(2 * a, (a * a).sum(1))


def queries(kind, n) -> dict:
    """dict(q f32[Q,3] and the slices of its parts), in this order: 300 uniform in the bounding box enlarged by 10 %, 20
    sites, up to 20 midpoints of list edges that float32 holds exactly and whose two ends are the midpoint's nearest sites
    (exact two-way ties), 20 circumcentres of Delaunay tetrahedra rounded to float32, 10 points 1e3 box sizes away, one
    NaN, one +inf; computed once and shared"""
    if (kind, n) in _QUERIES:
        return _QUERIES[(kind, n)]
    m = cloud(kind, n)
    pts, simplices = m["points"], m["simplices"]
    count = len(pts)
    rng = np.random.default_rng(2000 + n + 7 * len(kind))
    lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    pad = 0.05 * (hi - lo)
    box = rng.uniform(lo - pad, hi + pad, (300, 3)).astype(np.float32)
    sites = pts[rng.choice(count, 20, replace=False)]
    mids = []
    for i in rng.permutation(count):
        for j in row(m, i):
            mid = (pts[i].astype(np.float64) + pts[j].astype(np.float64)) / 2
            if i < j and len(mids) < 20 and (mid.astype(np.float32).astype(np.float64) == mid).all():
                tied = nearest_sites(pts, mid.astype(np.float32))
                if len(tied) == 2 and set(tied.tolist()) == {int(i), int(j)}:
                    mids.append(mid.astype(np.float32))
        if len(mids) == 20:
            break
    assert len(mids) >= 10, (kind, n, len(mids))
    chosen = simplices[rng.choice(len(simplices), 20, replace=False)]
    centres = np.array([_circumcentre(pts[s].astype(np.float64)) for s in chosen]).astype(np.float32)
    away = rng.normal(size=(10, 3))
    far = ((lo + hi) / 2 + 1e3 * np.linalg.norm(hi - lo) * away / np.linalg.norm(away, axis=1, keepdims=True)).astype(np.float32)
    parts = [("uniform", box), ("sites", sites), ("mids", np.array(mids, dtype=np.float32).reshape(-1, 3)),
             ("centres", centres), ("far", far), ("nan", np.array([[np.nan, 0.0, 0.0]], dtype=np.float32)),
             ("inf", np.array([[0.0, np.inf, 0.0]], dtype=np.float32))]
    out, at = {}, 0
    for name, part in parts:
        out[name] = slice(at, at + len(part))
        at += len(part)
    out["q"] = np.ascontiguousarray(np.concatenate([part for _, part in parts]))
    _QUERIES[(kind, n)] = out
    return out


def given_starts(kind, n):
    """a start per query, anywhere in the cloud"""
    return np.random.default_rng(n + len(kind)).integers(0, len(cloud(kind, n)["points"]), len(queries(kind, n)["q"]))


def valid_queries(m):
    lo, hi = m["points"].min(0), m["points"].max(0)
    return np.random.default_rng(5).uniform(lo, hi, (40, 3)).astype(np.float32)


# ---- stale and malformed lists --------------------------------------------------------------------------------------------

def stale(m, seed=9):
    """(adjacency, offsets) with 5 % of the entries deleted at random: only the local-minimum guarantee holds"""
    adj, off = m["adjacency"].astype(np.int64), m["offsets"].astype(np.int64)
    keep = np.random.default_rng(seed).uniform(size=len(adj)) >= 0.05
    owner = np.repeat(np.arange(len(off) - 1), np.diff(off))
    return adj[keep].astype(np.uint32), np.searchsorted(owner[keep], np.arange(len(off))).astype(np.uint32)


def malformed(m, i=7) -> dict:
    """name -> (adjacency, offsets, start, queries), int64 lists: each a RuntimeError of the walks from ``start``"""
    n = len(m["points"])
    adj, off = m["adjacency"].astype(np.int64), m["offsets"].astype(np.int64)
    q = valid_queries(m)
    at = np.full(len(q), i, dtype=np.int64)
    outside = at.copy()
    outside[3] = n
    backwards = off.copy()
    backwards[[i, i + 1]] = backwards[[i + 1, i]]
    past = off.copy()
    past[-1] = len(adj) + 3
    above, below = adj.copy(), adj.copy()
    above[off[i] + 1], below[off[i + 1] - 1] = n, -1
    return {"start": (adj, off, outside, q), "offsets": (adj, backwards, at, q),
            "past": (adj, past, np.full(len(q), n - 1, dtype=np.int64), q), "above": (above, off, at, q),
            "below": (below, off, at, q)}
