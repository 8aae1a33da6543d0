"""The reference of the cell-geometry gradient tests: difference quotients of the exact rational geometry
(tests/cell_geometry_ref.exact_geometry), with their own error measured.

For a cloud and upstreams (w, u) let  L = sum over the chosen bounded cells of  w_a V_a + u_a . c_a,  an exact Fraction.
The clouds are those of tests/host_harness/clip_host with every coordinate rounded to a multiple of 2^-16 (all have
|x| < 16), and the steps are integer multiples of 2^-20, so every perturbed coordinate is an fp32 number and the
difference quotient itself is exact.  For an integer direction delta, with h = 2^-19,

    D(h) = (L(p + h delta) - L(p - h delta)) / (2 h),   R = (4 D(h/2) - D(h)) / 3,   spread = |D(h/2) - D(h)|.

R is the reference value of <grad, delta> and the spread its uncertainty: the bar of the tests is |<grad, delta> - R| <=
spread, under the condition -- on the reference alone -- that spread <= 1e-3 max |R| over the case's probes.  V and
M = V c are C^1 across Delaunay flips (a face that appears or vanishes has zero area at the flip), so the quotients
converge whether or not a flip falls inside the step.

Nothing here shares code or numerics with radfoam_amd/csrc/rf_clip_grad.hpp.

A case costs about a hundred exact geometries (half a minute to a minute), so R and spread of every case are also
recorded in tests/golden/cell_geometry_grad/fd.npz (``python -m tests.cell_geometry_grad_ref`` writes it from the host
forward's bounded cells).  The CPU test computes each reference afresh and requires the record to equal it bit for bit;
the GPU tests read the record (recorded()).
"""
from __future__ import annotations

import math
import os
from fractions import Fraction

import numpy as np

from tests import cell_geometry_ref as X
from tests.host_harness import clip_host as H

GRID_BITS = 16            # coordinates are multiples of 2^-16
STEP = 2.0 ** -19         # h; h / 2 = 2^-20 is the unit every perturbed coordinate is a multiple of
REFERENCE_SPREAD = 1e-3   # a reference whose two step sizes disagree by more than this (of max |R|) is not a reference

FD_CASES = ("uniform400", "hub64", "hub65", "ring16", "ring17", "redo_spread")
_CASES = {}
_REFS = {}
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cell_geometry_grad", "fd.npz")


def rounded(points: np.ndarray) -> np.ndarray:
    p = points.astype(np.float64)
    assert np.abs(p).max() < 16.0
    out = (np.round(p * 2.0 ** GRID_BITS) / 2.0 ** GRID_BITS).astype(np.float32)
    assert np.array_equal(out.astype(np.float64) * 2.0 ** GRID_BITS, np.round(p * 2.0 ** GRID_BITS))
    return out


def case(name: str) -> dict:
    """The clip_host cloud ``name`` on the 2^-16 grid: points, Qhull's CSR, rows, and the exact reference."""
    if name not in _CASES:
        from radfoam_amd import foam

        pts = rounded(H._CLOUDS[name]())
        off, adj = foam.delaunay_csr(pts)
        _CASES[name] = dict(points=pts, offsets=off, adjacency=adj, exact=X.exact_geometry(pts),
                            rows=np.repeat(np.arange(pts.shape[0]), np.diff(off.astype(np.int64))))
    return _CASES[name]


def faces_of(c: dict, a: int):
    """the exact reference's faces of site a: {b: (area, distinct vertices, extent)}"""
    return {(q if p == a else p): f for (p, q), f in c["exact"]["faces"].items() if a in (p, q)}


def upstreams(c: dict, cells: np.ndarray, seed: int = 0):
    """(w f64[N], u f64[N,3]): w_a = r_a / s_a^2 and u_a = r'_a with r, r' uniform in [-1,1] and s_a = V_a^(1/3), so that
    every cell's own term of its row is O(1); zero outside ``cells`` (bool[N])."""
    rng = np.random.default_rng(seed)
    n = len(c["points"])
    size = np.cbrt(np.where(cells, c["exact"]["volume_f"], 1.0))
    w = np.where(cells, rng.uniform(-1.0, 1.0, n) / size ** 2, 0.0)
    u = np.where(cells[:, None], rng.uniform(-1.0, 1.0, (n, 3)), 0.0)
    return w, u


def exact_loss(points: np.ndarray, w: np.ndarray, u: np.ndarray, cells: np.ndarray) -> Fraction:
    ex = X.exact_geometry(points)
    X._CACHE.pop((points.shape, points.tobytes()), None)     # one of hundreds of perturbed clouds: not worth keeping
    total = Fraction(0)
    for a in np.nonzero(cells)[0]:
        assert not ex["open"][a], f"cell {a} opened under the perturbation"
        total += Fraction(float(w[a])) * ex["volume"][a]
        total += sum(Fraction(float(u[a, k])) * ex["centroid"][a][k] for k in range(3))
    return total


def quotient(points: np.ndarray, delta: np.ndarray, w, u, cells):
    """(R, spread) for the integer direction delta i64[N,3]"""
    assert delta.dtype == np.int64
    out = []
    for h in (STEP, 0.5 * STEP):
        step = delta.astype(np.float64) * h
        plus, minus = (points.astype(np.float64) + step).astype(np.float32), (points.astype(np.float64) - step).astype(np.float32)
        assert np.array_equal(plus.astype(np.float64) - points, step) and np.array_equal(points - minus.astype(np.float64), step)
        diff = exact_loss(plus, w, u, cells) - exact_loss(minus, w, u, cells)
        out.append(float(diff / Fraction(2.0 * h)))
    d1, d2 = out
    return (4.0 * d2 - d1) / 3.0, abs(d2 - d1)


def directions(c: dict, seams, count: int = 6, seed: int = 1):
    """``count`` random integer directions (every coordinate of every site in -3..3) and one single-coordinate probe
    (site, axis) per entry of ``seams``"""
    rng = np.random.default_rng(seed)
    n = len(c["points"])
    out = [rng.integers(-3, 4, size=(n, 3), dtype=np.int64) for _ in range(count)]
    for site, axis in seams:
        d = np.zeros((n, 3), dtype=np.int64)
        d[site, axis] = 1
        out.append(d)
    return out


SEAM_PROBES = {"uniform400": (), "hub64": ((0, 0), (1, 1)), "hub65": ((0, 2), (1, 0)), "ring16": ((0, 2), (1, 0)),
               "ring17": ((0, 0), (1, 2)), "redo_spread": ((0, 2), (73, 0), (200, 1))}


def reference(name: str, cells: np.ndarray) -> dict:
    """The difference-quotient reference of case ``name`` for L over ``cells``: w, u, the probes' directions, R and
    spread per probe.  Computed once per process and never modified; asserts the condition on the reference."""
    key = (name, cells.tobytes())
    if key not in _REFS:
        c = case(name)
        assert not c["exact"]["open"][cells].any()
        w, u = upstreams(c, cells)
        dirs = directions(c, SEAM_PROBES[name])
        got = [quotient(c["points"], d, w, u, cells) for d in dirs]
        R, spread = np.array([g[0] for g in got]), np.array([g[1] for g in got])
        worst = spread.max() / np.abs(R).max()
        print(f"{name}: reference spread / max |R| = {worst:.3g} over {len(dirs)} probes (max |R| = {np.abs(R).max():.4g})")
        assert worst <= REFERENCE_SPREAD
        _REFS[key] = dict(w=w, u=u, directions=dirs, R=R, spread=spread, worst=worst)
    return _REFS[key]


def recorded(name: str) -> dict:
    """reference() as recorded in tests/golden: cells, w, u, directions, R, spread (w, u and the directions are derived
    again from the recorded cells; they are functions of the case and its seeds)"""
    with np.load(_GOLDEN) as z:
        cells, R, spread = z[name + "_cells"], z[name + "_R"], z[name + "_spread"]
    c = case(name)
    assert not c["exact"]["open"][cells].any()
    w, u = upstreams(c, cells)
    assert (spread <= REFERENCE_SPREAD * np.abs(R).max()).all()
    return dict(cells=cells, w=w, u=u, directions=directions(c, SEAM_PROBES[name]), R=R, spread=spread)


def check_against_reference(name: str, ref: dict, grad: np.ndarray):
    """the bar: |<grad, delta> - R| <= spread on every probe"""
    got = np.array([(grad * d).sum() for d in ref["directions"]])
    miss = np.abs(got - ref["R"])
    for g, r, s, m in zip(got, ref["R"], ref["spread"], miss):
        print(f"{name}: <grad, delta> = {g:+.12e}, R = {r:+.12e}, |difference| = {m:.3g}, spread = {s:.3g}")
    assert np.isfinite(got).all() and (miss <= ref["spread"]).all()


def exact_face(points: np.ndarray, a: int, b: int):
    """(area, centroid f64[3]) of the Voronoi face of the Delaunay edge (a,b), bounded, from the circumcentres of the
    tetrahedra around the edge as Fractions."""
    from scipy.spatial import Delaunay

    tri = Delaunay(points.astype(np.float64))
    tets, nbrs = tri.simplices.tolist(), tri.neighbors.tolist()
    fr = [[Fraction(float(x)) for x in row] for row in points]
    scale = max(f.denominator for row in fr for f in row)
    P = [tuple(int(f * scale) for f in row) for row in fr]
    t0 = next(t for t, tet in enumerate(tets) if a in tet and b in tet)
    cyc = X._cycle(tets, nbrs, t0, a, b)
    assert cyc is not None
    cc = [X._circumcentre(*(P[v] for v in tets[t])) for t in cyc]
    vs = [tuple(Fraction(n[k], D) for k in range(3)) for n, D in (c for c in cc if c is not None)]
    d = X._sub(P[b], P[a])
    S, M = Fraction(0), [Fraction(0)] * 3
    for i in range(1, len(vs) - 1):
        tau = X._dot(X._cross(X._sub(vs[i], vs[0]), X._sub(vs[i + 1], vs[0])), d)
        S += tau
        M = [M[k] + tau * (vs[0][k] + vs[i][k] + vs[i + 1][k]) for k in range(3)]
    assert S != 0
    area = float(abs(S) / (2 * scale * scale)) / math.sqrt(X._dot(d, d))
    return area, np.array([float(M[k] / (3 * S) / scale) for k in range(3)])


if __name__ == "__main__":
    from tests.host_harness import clip_grad_host as HG

    out = {}
    for name in FD_CASES:
        cells = HG.host_forward(("rounded", name), case(name))["bounded"]
        ref = reference(name, cells)
        out.update({name + "_cells": cells, name + "_R": ref["R"], name + "_spread": ref["spread"]})
    np.savez(_GOLDEN, **out)
