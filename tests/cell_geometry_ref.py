"""Exact Voronoi cell geometry, in rational arithmetic: the reference of the cell-geometry tests.

The fp32 points are exact dyadic rationals; scaled by a power of two they are integers.  scipy.spatial.Delaunay gives the
tetrahedra (combinatorics only).  The Voronoi vertices are the tetrahedra's circumcentres, rational by Cramer's rule; the
face of a Delaunay edge (a,b) is the polygon of the circumcentres of the tetrahedra around the edge, ordered by walking
tetrahedron adjacency.  With v_0..v_{m-1} that polygon and d = p_b - p_a,

    S = sum_i ((v_i - v_0) x (v_{i+1} - v_0)) . d      (= 2 A_ab . d)
    M = sum_i tau_i (v_0 + v_i + v_{i+1})               (3 S times the face's area centroid)

are rational; the face's pyramid over either site has volume |S| / 12 and its centroid 3/4 of the way from the site to
M / (3 S), so a cell's volume and centroid are exact Fractions.  A face's area |S| / (2 |d|) takes one square root.  A
cell is open exactly when its site is on the hull of the triangulation.  Nothing here shares code or numerics with
radfoam_amd/csrc/rf_clip.hpp or with Qhull's Voronoi diagram; a tetrahedron that is flat in exact arithmetic (Qhull
triangulates cospherical sites with such) has no circumcentre and is left out of the polygons it would belong to, where
it would only repeat a vertex.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

_CACHE = {}


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _circumcentre(p0, p1, p2, p3):
    """of four integer points: (three integer numerators, their common denominator); None if they are coplanar"""
    d1, d2, d3 = _sub(p1, p0), _sub(p2, p0), _sub(p3, p0)
    c23, c31, c12 = _cross(d2, d3), _cross(d3, d1), _cross(d1, d2)
    det = _dot(d1, c23)
    if det == 0:
        return None
    r1, r2, r3 = _dot(d1, d1), _dot(d2, d2), _dot(d3, d3)
    den = 2 * det
    return tuple(den * p0[k] + r1 * c23[k] + r2 * c31[k] + r3 * c12[k] for k in range(3)), den


def _cycle(tets, nbrs, t0, a, b):
    """the tetrahedra around edge (a,b) in order, from t0; None if the edge is on the hull"""
    prev, pivot = [v for v in tets[t0] if v != a and v != b]
    t, out = t0, [t0]
    while True:
        t2 = nbrs[t][tets[t].index(prev)]
        if t2 < 0:
            return None
        if t2 == t0:
            return out
        new = [v for v in tets[t2] if v != a and v != b and v != pivot]
        assert len(new) == 1 and len(out) <= len(tets)
        prev, pivot = pivot, new[0]
        t = t2
        out.append(t)


def exact_geometry(points: np.ndarray) -> dict:
    """points: float32 [N,3], N >= 5 in general position enough for Qhull to keep every site.  Returns

      open        bool[N]          the site is a hull vertex
      volume      [N] Fraction     (None for an open cell);   volume_f   f64[N], +inf for an open cell
      centroid    [N] 3 Fractions  (None for an open cell);   centroid_f f64[N,3], NaN for an open cell
      extent      f64[N]           largest distance of a face vertex from its face's centre (p_a + p_b) / 2; +inf if open
      faces       {(a,b), a < b: (area, distinct vertices, extent)}  for every Delaunay edge; (inf, -1, inf) for an edge
                  on the hull, whose face is unbounded
      tets        the number of tetrahedra

    Computed once per array (keyed by its bytes) and never modified."""
    key = (points.shape, points.tobytes())
    if key in _CACHE:
        return _CACHE[key]
    from scipy.spatial import Delaunay

    assert points.dtype == np.float32
    n = points.shape[0]
    tri = Delaunay(points.astype(np.float64))
    assert tri.coplanar.size == 0
    tets, nbrs = tri.simplices.tolist(), tri.neighbors.tolist()
    fr = [[Fraction(float(x)) for x in row] for row in points]
    scale = max(f.denominator for row in fr for f in row)
    P = [tuple(int(f * scale) for f in row) for row in fr]
    cc = [_circumcentre(*(P[v] for v in t)) for t in tets]

    is_open = np.zeros(n, dtype=bool)
    first = {}                                      # an edge's first tetrahedron
    for t, (tet, nb) in enumerate(zip(tets, nbrs)):
        for j in range(4):
            if nb[j] < 0:
                is_open[[tet[i] for i in range(4) if i != j]] = True
            for i in range(j):
                first.setdefault((min(tet[i], tet[j]), max(tet[i], tet[j])), t)

    vol = [Fraction(0)] * n
    mom = [(Fraction(0),) * 3 for _ in range(n)]    # sum over faces of sign(S) M / 48
    extent = np.zeros(n)
    faces = {}
    for (a, b), t0 in first.items():
        cyc = _cycle(tets, nbrs, t0, a, b)
        if cyc is None:
            assert is_open[a] and is_open[b]
            faces[(a, b)] = (math.inf, -1, math.inf)
            continue
        vs = [cc[t] for t in cyc if cc[t] is not None]       # (numerators, denominator): integers until a sum is due
        d = _sub(P[b], P[a])
        n0, D0 = vs[0]
        S, M = Fraction(0), [Fraction(0)] * 3
        rel = [tuple(n[k] * D0 - n0[k] * D for k in range(3)) for n, D in vs]     # (v_i - v_0) D_i D_0
        for i in range(1, len(vs) - 1):
            (ni, Di), (nj, Dj) = vs[i], vs[i + 1]
            num = _dot(_cross(rel[i], rel[i + 1]), d)
            if num != 0:
                den = Di * Dj * D0 * D0
                S += Fraction(num, den)
                den *= D0 * Di * Dj
                for k in range(3):
                    M[k] += Fraction(num * (n0[k] * Di * Dj + ni[k] * D0 * Dj + nj[k] * D0 * Di), den)
        sign = 1 if S >= 0 else -1
        mid = [0.5 * (P[a][k] + P[b][k]) for k in range(3)]
        reach = max(math.sqrt(sum((n[k] / D - mid[k]) ** 2 for k in range(3))) for n, D in vs) / scale
        area = float(Fraction(abs(S), 2 * scale * scale)) / math.sqrt(_dot(d, d))
        distinct = len({tuple(Fraction(n[k], D) for k in range(3)) for n, D in vs})
        faces[(a, b)] = (area, distinct, reach)
        for site in (a, b):
            vol[site] = vol[site] + abs(S) / 12
            mom[site] = tuple(mom[site][k] + sign * M[k] / 48 for k in range(3))
            extent[site] = max(extent[site], reach)

    volume, centroid = [None] * n, [None] * n
    volume_f, centroid_f = np.full(n, np.inf), np.full((n, 3), np.nan)
    for a in range(n):
        if is_open[a]:
            extent[a] = np.inf
            continue
        assert vol[a] > 0
        volume[a] = vol[a] / scale ** 3
        centroid[a] = tuple((mom[a][k] / vol[a] + Fraction(P[a][k], 4)) / scale for k in range(3))
        volume_f[a] = float(volume[a])
        centroid_f[a] = [float(x) for x in centroid[a]]
    out = dict(open=is_open, volume=volume, centroid=centroid, volume_f=volume_f, centroid_f=centroid_f,
               extent=extent, faces=faces, tets=len(tets))
    _CACHE[key] = out
    return out


def per_slot(ref: dict, offsets: np.ndarray, adjacency: np.ndarray) -> dict:
    """The faces of ``ref`` aligned with a CSR's adjacency slots: area f64[E] (+inf on the hull), vertices i64[E]
    (-1 on the hull), extent f64[E].  The CSR must list exactly the edges of the reference's triangulation."""
    off, adj = offsets.astype(np.int64), adjacency.astype(np.int64)
    rows = np.repeat(np.arange(len(off) - 1), np.diff(off))
    assert len(adj) == 2 * len(ref["faces"])
    got = [ref["faces"][(min(a, b), max(a, b))] for a, b in zip(rows.tolist(), adj.tolist())]   # KeyError: not an edge
    return dict(area=np.array([g[0] for g in got], dtype=np.float64).reshape(-1),
                vertices=np.array([g[1] for g in got], dtype=np.int64).reshape(-1),
                extent=np.array([g[2] for g in got], dtype=np.float64).reshape(-1))
