"""Exact second moments of Voronoi cells clipped to an axis-aligned box, in rational arithmetic: the reference of the
tests of radfoam.cell_moments_in_box.

The plane list of tests/cell_box_ref.py: relative to p_a, cell_box(a) is the intersection of the half-spaces  n_j . y <=
h_j  of a's adjacency row (n = p_b - p_a, h = |n|^2 / 2, in row order) and of the six walls (n a signed axis vector, h the
signed distance, in wall order).  The face on plane i is found in the plane's rational, orthogonal but not normalised
basis  u = n x e, v = n x u  about  c = n h / |n|^2:  a square that covers the box, counter-clockwise about n, is cut by
every other half-space with Fractions; of two planes of the list that are the same plane with the same outward side the
earlier keeps the face.  The polygon's exact 3-D vertices are  Y_i = c + s_i u + t_i v,  and the face's pyramid over the
site is the fan of tetrahedra (0, Y_0, Y_i, Y_{i+1}); a tetrahedron (0, P, Q, R) with det = P . (Q x R) has

    volume det / 6,    int y dy = det / 24 S,    int y y^T dy = det / 120 (S S^T + P P^T + Q Q^T + R R^T),    S = P + Q + R.

The determinant is taken with its sign: the polygon is counter-clockwise about n, so the sign is that of h, negative for a
wall the site lies outside of, and the signed sum over the list is the integral over cell(a) n box wherever the site is.
The volume and the first moment come from the same polygons, and the central moment  Q - M M^T / V  from them.  Nothing
here shares arithmetic with radfoam_amd/csrc: no unit frames, no 2-D polygon moments, no square roots, no rounding.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

from tests.cell_box_ref import _clip, _cross, _dot

_CACHE = {}
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))          # xx, yy, zz, xy, xz, yz


def _face_vertices(planes, i, reach):
    """the exact 3-D vertices, relative to the site, of the face on plane i of the list; counter-clockwise about n_i"""
    n, h = planes[i]
    k = min(range(3), key=lambda q: abs(n[q]))
    u = _cross(n, tuple(Fraction(int(q == k)) for q in range(3)))
    v = _cross(n, u)
    nn, uu, vv = _dot(n, n), _dot(u, u), _dot(v, v)
    c = tuple(x * h / nn for x in n)
    L = Fraction(int(reach / math.sqrt(float(min(uu, vv)))) + 2)
    poly = [((x, y), (float(x), float(y))) for x, y in ((-L, -L), (L, -L), (L, L), (-L, L))]
    uf, vf, cf = [float(x) for x in u], [float(x) for x in v], [float(x) for x in c]
    for j, (d, hj) in enumerate(planes):
        if j == i or not poly:
            continue
        # A plane that every vertex is inside of by far more than doubles can be wrong about leaves the polygon as it is,
        # and its Fractions are not formed: the floats' rounding error is below 1e-14 of ``mag``, the margin 1e-9 of it.
        # A coincident plane has e == 0 at every vertex and never passes.
        df, hf = [float(x) for x in d], float(hj)
        Af, Bf, Cf = _dot(df, uf), _dot(df, vf), hf - _dot(df, cf)
        Am, Bm = sum(abs(df[q] * uf[q]) for q in range(3)), sum(abs(df[q] * vf[q]) for q in range(3))
        Cm = abs(hf) + sum(abs(df[q] * cf[q]) for q in range(3))
        if all(Af * sf + Bf * tf - Cf < -1e-9 * (Am * abs(sf) + Bm * abs(tf) + Cm) for _, (sf, tf) in poly):
            continue
        A, B, C = _dot(d, u), _dot(d, v), hj - _dot(d, c)
        if A == 0 and B == 0 and C == 0 and _dot(d, n) > 0:      # the plane of face i itself: the earlier keeps it
            if j < i:
                poly = []
            continue
        poly = _clip(poly, A, B, C)
    return [tuple(c[q] + s * u[q] + t * v[q] for q in range(3)) for (s, t), _ in poly]


def cell_sums(planes, reach):
    """planes: [(n, h)] in Fractions relative to the site.  Returns (volume, first moment [3], second moment [6]) of the
    intersection of the half-spaces, about the site, as Fractions."""
    det_sum, first, second = Fraction(0), [Fraction(0)] * 3, [Fraction(0)] * 6
    for i in range(len(planes)):
        Y = _face_vertices(planes, i, reach)
        for a in range(1, len(Y) - 1):
            P, Q, R = Y[0], Y[a], Y[a + 1]
            det = _dot(P, _cross(Q, R))
            if det == 0:
                continue
            assert (det > 0) == (planes[i][1] > 0)
            S = tuple(P[q] + Q[q] + R[q] for q in range(3))
            det_sum += det
            first = [first[q] + det * S[q] for q in range(3)]
            second = [second[k] + det * (S[i0] * S[i1] + P[i0] * P[i1] + Q[i0] * Q[i1] + R[i0] * R[i1])
                      for k, (i0, i1) in enumerate(PAIRS)]
    return det_sum / 6, [x / 24 for x in first], [x / 120 for x in second]


def planes_of(P, lo, hi, row, a):
    planes = []
    for b in row:
        d = tuple(P[b][q] - P[a][q] for q in range(3))
        planes.append((d, _dot(d, d) / 2))
    for k in range(3):
        planes.append((tuple(Fraction(-int(q == k)) for q in range(3)), P[a][k] - lo[k]))
        planes.append((tuple(Fraction(int(q == k)) for q in range(3)), hi[k] - P[a][k]))
    return planes


def exact_moments_in_box(points: np.ndarray, offsets: np.ndarray, adjacency: np.ndarray, box, cells) -> dict:
    """points float32 [N,3], a CSR, box = six floats (lo, hi) taken exactly, cells = the cells to work on.  Returns, with
    None / NaN / False outside ``cells``,

      done        bool[N]
      volume      {a: Fraction}, first {a: 3 Fractions} (int y dy), site {a: 6 Fractions}, central {a: 6 Fractions or None
                  where the volume is 0}
      volume_f    f64[N]; site_f, central_f  f64[N,6] (central NaN where the volume is 0)
      trace_f     f64[N]  tr site, the unit of the tests' bar; trace_central_f  f64[N]  tr central

    Computed once per argument set and never modified."""
    assert points.dtype == np.float32
    six = [float(x) for x in np.asarray(box, dtype=np.float64).reshape(-1)]
    cells = tuple(int(a) for a in cells)
    key = (points.tobytes(), np.asarray(adjacency).tobytes(), np.asarray(offsets).tobytes(), tuple(six), cells)
    if key in _CACHE:
        return _CACHE[key]
    n, off, adj = len(points), np.asarray(offsets).astype(np.int64), np.asarray(adjacency).astype(np.int64)
    P = [tuple(Fraction(float(x)) for x in row) for row in points]
    lo, hi = [Fraction(x) for x in six[:3]], [Fraction(x) for x in six[3:]]
    allmin = np.minimum(points.min(0).astype(np.float64), six[:3])
    allmax = np.maximum(points.max(0).astype(np.float64), six[3:])
    reach = 2.0 * float(np.linalg.norm(allmax - allmin))
    out = dict(done=np.zeros(n, dtype=bool), volume={}, first={}, site={}, central={}, volume_f=np.full(n, np.nan),
               site_f=np.full((n, 6), np.nan), central_f=np.full((n, 6), np.nan), trace_f=np.full(n, np.nan),
               trace_central_f=np.full(n, np.nan))
    for a in cells:
        volume, first, second = cell_sums(planes_of(P, lo, hi, adj[off[a]:off[a + 1]].tolist(), a), reach)
        assert volume >= 0
        out["done"][a] = True
        out["volume"][a], out["first"][a], out["site"][a] = volume, first, second
        out["volume_f"][a] = float(volume)
        out["site_f"][a] = [float(x) for x in second]
        out["trace_f"][a] = float(second[0] + second[1] + second[2])
        if volume > 0:
            central = [second[k] - first[i] * first[j] / volume for k, (i, j) in enumerate(PAIRS)]
            out["central"][a] = central
            out["central_f"][a] = [float(x) for x in central]
            out["trace_central_f"][a] = float(central[0] + central[1] + central[2])
            assert out["trace_f"][a] > 0.0 and out["trace_central_f"][a] > 0.0
        else:
            assert all(x == 0 for x in second)
            out["central"][a] = None
    _CACHE[key] = out
    return out
