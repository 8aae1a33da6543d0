"""An independent reference of marching tetrahedra for the tests of radfoam.isosurface: no case table and no winding rule.

Per tetrahedron it collects the points where the level crosses the six edges, orders them cyclically around their centroid
and orients the polygon geometrically, so that its normal has a positive component along (mean of the outside sites - mean
of the inside sites).  It reports the set of the crossed edges and the polygon's area vector, which does not depend on how
a quad is cut in two: comparing both checks the case rule and the winding of the operator without copying them.

That direction w is never in the polygon's plane: the field is linear on the tetrahedron, its gradient g has
g . (p_out - p_in) < 0 for every outside/inside pair, so g . w < 0.  Projected along w the planar convex polygon keeps its
cyclic order, which is how the points are sorted.
"""
import itertools

import numpy as np


def tetrahedron(p, v, sites, level):
    """(set of (a, b) with a < b, area vector f64[3]) of one tetrahedron; p f64[N,3], v f64[N]"""
    vv = v[sites]
    inside = vv > level
    if not np.isfinite(vv).all() or inside.all() or not inside.any():
        return set(), np.zeros(3)
    keys, pts = [], []
    for x, y in itertools.combinations(range(4), 2):
        if inside[x] != inside[y]:
            a, b = sorted((int(sites[x]), int(sites[y])))
            t = (level - v[a]) / (v[b] - v[a])
            keys.append((a, b))
            pts.append(p[a] + t * (p[b] - p[a]))
    pts = np.array(pts)
    w = p[sites[~inside]].mean(0) - p[sites[inside]].mean(0)
    w /= np.linalg.norm(w)
    u1 = np.cross(w, np.eye(3)[np.argmin(np.abs(w))])
    u1 /= np.linalg.norm(u1)
    u2 = np.cross(w, u1)
    r = pts - pts.mean(0)
    r = r[np.argsort(np.arctan2(r @ u2, r @ u1))]              # counter-clockwise seen from +w
    area = 0.5 * np.cross(r, np.roll(r, -1, axis=0)).sum(0)
    if area @ w < 0:
        area = -area
    return set(keys), area


def reference(points, tets, values, level):
    """(list of key sets, area vectors f64[T,3]) over all tetrahedra, in float64 from the inputs as given"""
    p, v = np.asarray(points, dtype=np.float64), np.asarray(values, dtype=np.float64)
    tets = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    sets, areas = [], np.zeros((len(tets), 3))
    for t, sites in enumerate(tets):
        s, areas[t] = tetrahedron(p, v, sites, level)
        sets.append(s)
    return sets, areas
