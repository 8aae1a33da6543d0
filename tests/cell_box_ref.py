"""Exact geometry of Voronoi cells clipped to an axis-aligned box, in rational arithmetic: the reference of the tests of
radfoam.cell_geometry_in_box.

The fp32 points and the box's doubles are exact rationals.  Relative to p_a, cell_box(a) is the intersection of the
half-spaces  n_j . y <= h_j  of a's adjacency row (n = p_b - p_a, h = |n|^2 / 2, in row order) and of the six walls (n a
signed axis vector, h the signed distance, in wall order).  The face on plane i is found in the plane's own rational,
orthogonal but not normalised basis  u = n x e, v = n x u  (e the axis n leans on least) about c = n h / |n|^2: a square
that covers the box is cut by every other half-space with Fractions, so every vertex is the exact intersection it stands
for.  With Q the polygon's area in (s,t),

    area vector  = Q |u|^2 n            (u x v = |u|^2 n)
    pyramid      = Q |u|^2 h / 3        (rational; signed with h)
    face area    = Q |u|^2 |n|          (one square root)

and the cell's volume and centroid are sums of rationals.  Coincident planes follow the definition: of two planes of the
list that are the same plane with the same outward side, the earlier keeps the face.  Nothing here shares code or numerics
with radfoam_amd/csrc/rf_clip_box.hpp: other frames, no square roots before the end, no rounding.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

_CACHE = {}


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _clip(poly, A, B, C):
    """The part of the polygon with A s + B t <= C; a vertex on the line is inside and is not emitted twice.  A vertex is
    ((s, t) Fractions, (s, t) floats).  The floats only ever decide on which side a vertex lies, and only where it is off
    the line by more than 1e-10 of the terms' magnitudes (their rounding error is below 1e-15 of it); every other sign,
    and every value a crossing is formed from, is exact."""
    Af, Bf, Cf = float(A), float(B), float(C)
    m = len(poly)
    exact = [None] * m

    def e(i):
        if exact[i] is None:
            (s, t), _ = poly[i]
            exact[i] = A * s + B * t - C
        return exact[i]

    inside = []
    for i, (_, (sf, tf)) in enumerate(poly):
        x, y = Af * sf, Bf * tf
        ef = x + y - Cf
        inside.append(ef < 0 if abs(ef) > 1e-10 * (abs(x) + abs(y) + abs(Cf)) else e(i) <= 0)
    if all(inside):
        return poly
    if not any(inside):
        return []
    out = []
    for i in range(m):
        j = (i + 1) % m
        if inside[i]:
            out.append(poly[i])
        if inside[i] != inside[j] and e(i) != 0 and e(j) != 0:
            w = e(i) / (e(i) - e(j))
            (si, ti), (sj, tj) = poly[i][0], poly[j][0]
            s, t = si + w * (sj - si), ti + w * (tj - ti)
            out.append(((s, t), (float(s), float(t))))
    return out


def _cell(planes, reach):
    """planes: [(n, h)] in Fractions relative to the site; reach: a float bound on the distance of any point of the box
    from any plane's centre.  Returns (volume, first moment about the site, [(area float, distinct vertices)])."""
    volume, moment, faces = Fraction(0), [Fraction(0)] * 3, []
    for i, (n, h) in enumerate(planes):
        k = min(range(3), key=lambda q: abs(n[q]))
        u = _cross(n, tuple(Fraction(int(q == k)) for q in range(3)))
        v = _cross(n, u)
        nn, uu, vv = _dot(n, n), _dot(u, u), _dot(v, v)
        c = tuple(x * h / nn for x in n)
        L = Fraction(int(reach / math.sqrt(float(min(uu, vv)))) + 2)
        poly = [((x, y), (float(x), float(y))) for x, y in ((-L, -L), (L, -L), (L, L), (-L, L))]
        for j, (d, hj) in enumerate(planes):
            if j == i or not poly:
                continue
            A, B, C = _dot(d, u), _dot(d, v), hj - _dot(d, c)
            if A == 0 and B == 0 and C == 0 and _dot(d, n) > 0:      # the plane of face i itself: the earlier keeps it
                if j < i:
                    poly = []
                continue
            poly = _clip(poly, A, B, C)
        poly = [exact for exact, _ in poly]
        distinct = len(set(poly))
        Q2, ms, mt = Fraction(0), Fraction(0), Fraction(0)               # twice the area, its first moments times 3
        for a in range(1, len(poly) - 1):
            ps, pt = poly[a][0] - poly[0][0], poly[a][1] - poly[0][1]
            qs, qt = poly[a + 1][0] - poly[0][0], poly[a + 1][1] - poly[0][1]
            cr = ps * qt - pt * qs
            Q2 += cr
            ms += cr * (ps + qs)
            mt += cr * (pt + qt)
        if Q2 == 0:
            faces.append((0.0, distinct))
            continue
        assert Q2 > 0
        cs, ct = poly[0][0] + ms / (3 * Q2), poly[0][1] + mt / (3 * Q2)
        centre = tuple(c[q] + cs * u[q] + ct * v[q] for q in range(3))
        pyramid = Q2 * uu * h / 6
        volume += pyramid
        moment = [moment[q] + pyramid * Fraction(3, 4) * centre[q] for q in range(3)]
        faces.append((math.sqrt(float(Q2 * Q2 * uu * uu * nn / 4)), distinct))
    return volume, moment, faces


def exact_cells_in_box(points: np.ndarray, offsets: np.ndarray, adjacency: np.ndarray, box, cells) -> dict:
    """points float32 [N,3], a CSR, box = six floats (lo, hi) taken exactly, cells = the cells to work on.  Returns, with
    NaN / -1 / False outside ``cells``,

      done           bool[N]
      volume         {a: Fraction};   volume_f f64[N]
      centroid_f     f64[N,3]         NaN where the volume is 0
      face_area      f64[E], face_vertices i64[E]      aligned with the adjacency
      wall_area      f64[N,6], wall_vertices i64[N,6]

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
    out = dict(done=np.zeros(n, dtype=bool), volume={}, volume_f=np.full(n, np.nan), centroid_f=np.full((n, 3), np.nan),
               face_area=np.full(len(adj), np.nan), face_vertices=np.full(len(adj), -1, dtype=np.int64),
               wall_area=np.full((n, 6), np.nan), wall_vertices=np.full((n, 6), -1, dtype=np.int64))
    for a in cells:
        planes = []
        for b in adj[off[a]:off[a + 1]]:
            d = tuple(P[b][q] - P[a][q] for q in range(3))
            planes.append((d, _dot(d, d) / 2))
        for k in range(3):
            planes.append((tuple(Fraction(-int(q == k)) for q in range(3)), P[a][k] - lo[k]))
            planes.append((tuple(Fraction(int(q == k)) for q in range(3)), hi[k] - P[a][k]))
        volume, moment, faces = _cell(planes, reach)
        assert volume >= 0
        deg = int(off[a + 1] - off[a])
        out["done"][a] = True
        out["volume"][a] = volume
        out["volume_f"][a] = float(volume)
        if volume > 0:
            out["centroid_f"][a] = [float(P[a][q] + moment[q] / volume) for q in range(3)]
        out["face_area"][off[a]:off[a + 1]] = [f[0] for f in faces[:deg]]
        out["face_vertices"][off[a]:off[a + 1]] = [f[1] for f in faces[:deg]]
        out["wall_area"][a] = [f[0] for f in faces[deg:]]
        out["wall_vertices"][a] = [f[1] for f in faces[deg:]]
    _CACHE[key] = out
    return out
