"""Exact second moments of the Voronoi cells, in rational arithmetic: the reference of the cell-moment tests.

The construction of tests/cell_geometry_ref.py: the fp32 points scaled to integers, scipy.spatial.Delaunay for the
combinatorics, the rational circumcentres as Voronoi vertices, the face of a Delaunay edge (a,b) the polygon v_0..v_{m-1}
of the circumcentres around the edge.  Relative to site a, y_i = v_i - p_a, the face's pyramid over the site is the fan of
tetrahedra (0, y_0, y_i, y_{i+1}), and a tetrahedron (0, p, q, r) with det = p . (q x r) has

    int x x^T dx = det / 120 (s s^T + p p^T + q q^T + r r^T),   s = p + q + r

(the second moment of a simplex from its vertices and their sum; volume det / 6).  The face's fan is oriented by the sign
of its summed determinant: the site is inside its cell, so every pyramid counts positive.  The sum over a site's faces is
int_{cell} y y^T dy exactly; the central moment subtracts V m m^T with the exact volume and centroid of
cell_geometry_ref.exact_geometry.  Nothing here shares arithmetic with radfoam_amd/csrc/rf_clip*.hpp: no planes, no
clipping, no 2-D frames, no polygon moments.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

from tests import cell_geometry_ref as X
from tests.cell_geometry_ref import _circumcentre, _cross, _cycle, _dot

_CACHE = {}
_PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))          # xx, yy, zz, xy, xz, yz


def _fan_moment(ys):
    """sum over the fan (0, y_0, y_i, y_{i+1}) of det (s s^T + ...) for integer y: (six integers, summed det); the caller
    divides by 120 and by the fifth power of the y's common denominator"""
    acc, total = [0] * 6, 0
    p = ys[0]
    for i in range(1, len(ys) - 1):
        q, r = ys[i], ys[i + 1]
        det = _dot(p, _cross(q, r))
        if det == 0:
            continue
        s = (p[0] + q[0] + r[0], p[1] + q[1] + r[1], p[2] + q[2] + r[2])
        total += det
        for k, (i0, i1) in enumerate(_PAIRS):
            acc[k] += det * (s[i0] * s[i1] + p[i0] * p[i1] + q[i0] * q[i1] + r[i0] * r[i1])
    return acc, total


def exact_moments(points: np.ndarray, cells=None) -> dict:
    """points: float32 [N,3] as for exact_geometry.  ``cells``: the sites to work on (all by default).  Returns

      open       bool[N]           the site is a hull vertex
      done       bool[N]           the site was worked on and its cell is bounded
      site       [N] 6 Fractions   int y y^T dy, y = x - p_a, as xx, yy, zz, xy, xz, yz (None unless done)
      central    [N] 6 Fractions   about the exact centroid (None unless done)
      site_f, central_f   f64[N,6] the same rounded, NaN unless done
      trace_f    f64[N]            tr site, the unit of the tests' bar; NaN unless done

    Computed once per (array, cells) and never modified."""
    pick = None if cells is None else tuple(sorted(int(c) for c in cells))
    key = (points.shape, points.tobytes(), pick)
    if key in _CACHE:
        return _CACHE[key]
    from scipy.spatial import Delaunay

    assert points.dtype == np.float32
    n = points.shape[0]
    geo = X.exact_geometry(points)
    tri = Delaunay(points.astype(np.float64))
    assert tri.coplanar.size == 0
    tets, nbrs = tri.simplices.tolist(), tri.neighbors.tolist()
    fr = [[Fraction(float(x)) for x in row] for row in points]
    scale = max(f.denominator for row in fr for f in row)
    P = [tuple(int(f * scale) for f in row) for row in fr]
    wanted = np.ones(n, dtype=bool) if pick is None else np.isin(np.arange(n), pick)

    is_open = np.zeros(n, dtype=bool)
    first = {}
    for t, (tet, nb) in enumerate(zip(tets, nbrs)):
        for j in range(4):
            if nb[j] < 0:
                is_open[[tet[i] for i in range(4) if i != j]] = True
            for i in range(j):
                first.setdefault((min(tet[i], tet[j]), max(tet[i], tet[j])), t)
    assert np.array_equal(is_open, geo["open"])
    done = wanted & ~is_open

    cc = {}
    acc = {a: [Fraction(0)] * 6 for a in np.nonzero(done)[0].tolist()}
    for (a, b), t0 in first.items():
        if not (done[a] or done[b]):
            continue
        cyc = _cycle(tets, nbrs, t0, a, b)
        assert cyc is not None          # a bounded cell has no face on the hull
        vs = []
        for t in cyc:
            if t not in cc:
                c = _circumcentre(*(P[v] for v in tets[t]))
                cc[t] = c                      # (three integer numerators, their common denominator)
            if cc[t] is not None:
                vs.append(cc[t])
        den = math.lcm(*(D for _, D in vs))          # the polygon on one denominator: integers until the sum is due
        for site in (a, b):
            if not done[site]:
                continue
            ys = [tuple(num[k] * (den // D) - P[site][k] * den for k in range(3)) for num, D in vs]
            part, total = _fan_moment(ys)
            sign = 1 if total >= 0 else -1
            acc[site] = [acc[site][k] + Fraction(sign * part[k], den ** 5) for k in range(6)]

    site, central = [None] * n, [None] * n
    site_f, central_f, trace_f = np.full((n, 6), np.nan), np.full((n, 6), np.nan), np.full(n, np.nan)
    unit = Fraction(1, 120 * scale ** 5)
    for a, sums in acc.items():
        site[a] = tuple(x * unit for x in sums)
        m = tuple(geo["centroid"][a][k] - fr[a][k] for k in range(3))
        central[a] = tuple(site[a][k] - geo["volume"][a] * m[i] * m[j] for k, (i, j) in enumerate(_PAIRS))
        site_f[a] = [float(x) for x in site[a]]
        central_f[a] = [float(x) for x in central[a]]
        trace_f[a] = float(site[a][0] + site[a][1] + site[a][2])
        assert trace_f[a] > 0.0
    out = dict(open=is_open, done=done, site=site, central=central, site_f=site_f, central_f=central_f, trace_f=trace_f)
    _CACHE[key] = out
    return out
