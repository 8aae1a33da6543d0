"""The reference of the face-area gradient tests: difference quotients of the exact Voronoi face areas, with their own
error measured, by the method of tests/cell_geometry_grad_ref.py (same clouds on the 2^-16 grid, same directions and seam
probes, h = 2^-19, R = (4 D(h/2) - D(h)) / 3, spread = |D(h/2) - D(h)|).

The loss is  L = sum G_ab A_ab  over the faces {a,b} of finite exact area between two closed cells of the unperturbed
cloud that the forward under test calls finite too (``keep``; see kept()), G_ab = r / cbrt(min(V_a, V_b)) with r uniform
in [-1,1] from a fixed seed, one draw per face of finite exact area between closed cells in the order of (a,b), a < b.
A face's area is |S| / (2 |d|) from the exact S = 2 A |d| (tests/cell_geometry_ref.py) and the integer |d|^2;
sqrt(|d|^2) is math.isqrt of |d|^2 * 2^512 over 2^256, so L is a Fraction whose rounding (relative 2^-256) is far below
the spread.  A face the perturbation flips away has area 0; one it flips in has no weight.  Areas are C^1 across flips
(the face that comes or goes has area O(eps^2)), so the quotients converge whether or not a flip falls in the step.

Nothing here shares code or numerics with radfoam_amd/csrc/rf_clip_area_grad.hpp.

R and spread of every case are recorded in tests/golden/face_area_grad/fd.npz (``python -m tests.face_area_grad_ref``
writes it).  The CPU test computes each reference afresh and requires the record to equal it bit for bit; the GPU tests
read the record (recorded()).
"""
from __future__ import annotations

import math
import os
from fractions import Fraction

import numpy as np

from tests import cell_geometry_grad_ref as G
from tests import cell_geometry_ref as X

FD_CASES, SEAM_PROBES, STEP, REFERENCE_SPREAD = G.FD_CASES, G.SEAM_PROBES, G.STEP, G.REFERENCE_SPREAD
ROOT_BITS = 256           # sqrt(|d|^2) to 2^-256 of a unit of the scaled integers
_REFS = {}
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "face_area_grad", "fd.npz")

case, directions, check_against_reference = G.case, G.directions, G.check_against_reference


def exact_areas(points: np.ndarray, wanted):
    """({(a,b): area as a Fraction} for the pairs of ``wanted`` that are Delaunay edges off the hull, open bool[N]): the
    construction of cell_geometry_ref.exact_geometry (circumcentres around the edge), keeping S and |d|^2 exact."""
    from scipy.spatial import Delaunay

    assert points.dtype == np.float32
    tri = Delaunay(points.astype(np.float64))
    assert tri.coplanar.size == 0
    tets, nbrs = tri.simplices.tolist(), tri.neighbors.tolist()
    fr = [[Fraction(float(x)) for x in row] for row in points]
    scale = max(f.denominator for row in fr for f in row)
    P = [tuple(int(f * scale) for f in row) for row in fr]
    is_open = np.zeros(points.shape[0], dtype=bool)
    first = {}
    for t, (tet, nb) in enumerate(zip(tets, nbrs)):
        for j in range(4):
            if nb[j] < 0:
                is_open[[tet[i] for i in range(4) if i != j]] = True
            for i in range(j):
                first.setdefault((min(tet[i], tet[j]), max(tet[i], tet[j])), t)
    cc, out = {}, {}
    for a, b in wanted:
        t0 = first.get((a, b))
        cyc = None if t0 is None else X._cycle(tets, nbrs, t0, a, b)
        if cyc is None:
            continue
        for t in cyc:
            if t not in cc:
                cc[t] = X._circumcentre(*(P[v] for v in tets[t]))
        vs = [cc[t] for t in cyc if cc[t] is not None]
        d = X._sub(P[b], P[a])
        n0, D0 = vs[0]
        rel = [tuple(n[k] * D0 - n0[k] * D for k in range(3)) for n, D in vs]     # (v_i - v_0) D_i D_0
        S = Fraction(0)
        for i in range(1, len(vs) - 1):
            num = X._dot(X._cross(rel[i], rel[i + 1]), d)
            if num != 0:
                S += Fraction(num, vs[i][1] * vs[i + 1][1] * D0 * D0)
        dd = X._dot(d, d)
        root = Fraction(math.isqrt(dd << (2 * ROOT_BITS)), 1 << ROOT_BITS)        # sqrt(dd), rounded down
        out[(a, b)] = abs(S) * root / (2 * dd * scale * scale)
    return out, is_open


def faces_and_weights(c: dict, seed: int = 0):
    """(pairs [(a,b), a < b] in order, G f64[len(pairs)]): the faces of L and their weights"""
    ex = c["exact"]
    pairs = sorted(p for p, f in ex["faces"].items() if math.isfinite(f[0]) and not ex["open"][p[0]] and not ex["open"][p[1]])
    rng = np.random.default_rng(seed)
    v = np.array([min(ex["volume_f"][a], ex["volume_f"][b]) for a, b in pairs])
    return pairs, rng.uniform(-1.0, 1.0, len(pairs)) / np.cbrt(v)


def kept(c: dict, pairs, face_area: np.ndarray) -> np.ndarray:
    """bool[len(pairs)]: both slots of the face have a finite, positive area in the forward under test.  A face of a
    far-reaching cell next to the hull can be finite exactly and still reach past the forward's clipping square, where the
    forward calls it unbounded (+inf) by definition (tests/test_cell_geometry.py, "either way") and the gradient, which
    differentiates the forward, ignores it; such a face is no part of L (2 of uniform400's 2285, none elsewhere)."""
    slot = {(a, b): k for k, (a, b) in enumerate(zip(c["rows"].tolist(), c["adjacency"].astype(np.int64).tolist()))}
    ok = lambda k: math.isfinite(face_area[k]) and face_area[k] > 0.0
    return np.array([ok(slot[(a, b)]) and ok(slot[(b, a)]) for a, b in pairs])


def slot_upstream(c: dict, pairs, weights) -> np.ndarray:
    """g f64[E] whose effective weights are ``weights``: 3/4 of G_ab on the slot a -> b (a < b) and 1/4 on its mate (both
    exact in floating point), zero on every other slot"""
    w = {p: x for p, x in zip(pairs, weights.tolist())}
    rows, adj = c["rows"].tolist(), c["adjacency"].astype(np.int64).tolist()
    return np.array([0.75 * w.get((a, b), 0.0) if a < b else 0.25 * w.get((b, a), 0.0) for a, b in zip(rows, adj)])


def exact_loss(points: np.ndarray, pairs, weights) -> Fraction:
    areas, is_open = exact_areas(points, pairs)
    total = Fraction(0)
    for (a, b), w in zip(pairs, weights.tolist()):
        assert not is_open[a] and not is_open[b], f"cell {a} or {b} opened under the perturbation"
        total += Fraction(w) * areas.get((a, b), 0)
    return total


def quotient(points: np.ndarray, delta: np.ndarray, pairs, weights):
    """(R, spread) for the integer direction delta i64[N,3]"""
    assert delta.dtype == np.int64
    out = []
    for h in (STEP, 0.5 * STEP):
        step = delta.astype(np.float64) * h
        plus, minus = (points.astype(np.float64) + step).astype(np.float32), (points.astype(np.float64) - step).astype(np.float32)
        assert np.array_equal(plus.astype(np.float64) - points, step) and np.array_equal(points - minus.astype(np.float64), step)
        diff = exact_loss(plus, pairs, weights) - exact_loss(minus, pairs, weights)
        out.append(float(diff / Fraction(2.0 * h)))
    d1, d2 = out
    return (4.0 * d2 - d1) / 3.0, abs(d2 - d1)


def _host_keep(name):
    from tests.host_harness import clip_host as H

    c = case(name)
    return kept(c, faces_and_weights(c)[0], H.cell_geometry(c["points"], c["adjacency"], c["offsets"])["face_area"])


def _chosen(c, keep):
    pairs, weights = faces_and_weights(c)
    assert keep.shape == (len(pairs),) and keep.sum() >= 0.99 * len(pairs)
    return [p for p, k in zip(pairs, keep) if k], weights[keep]


def _probe(task):
    name, k = task
    c = case(name)
    pairs, weights = _chosen(c, _host_keep(name))
    return quotient(c["points"], directions(c, SEAM_PROBES[name])[k], pairs, weights)


def reference(name: str, keep: np.ndarray, got=None) -> dict:
    """The difference-quotient reference of case ``name`` over the faces ``keep`` (kept()): pairs, weights, the slot
    upstream g, the probes' directions, R and spread per probe.  Computed once per process and never modified; asserts
    the condition on the reference."""
    if name not in _REFS:
        c = case(name)
        pairs, weights = _chosen(c, keep)
        dirs = directions(c, SEAM_PROBES[name])
        if got is None:
            got = [quotient(c["points"], d, pairs, weights) for d in dirs]
        R, spread = np.array([g[0] for g in got]), np.array([g[1] for g in got])
        worst = spread.max() / np.abs(R).max()
        print(f"{name}: reference spread / max |R| = {worst:.3g} over {len(dirs)} probes (max |R| = {np.abs(R).max():.4g}, "
              f"{len(pairs)} faces)")
        assert worst <= REFERENCE_SPREAD
        _REFS[name] = dict(keep=keep, pairs=pairs, weights=weights, g=slot_upstream(c, pairs, weights), directions=dirs, R=R,
                           spread=spread, worst=worst)
    return _REFS[name]


def recorded(name: str) -> dict:
    """reference() as recorded in tests/golden (the faces, weights and directions are derived again: they are functions
    of the case and its seeds)"""
    with np.load(_GOLDEN) as z:
        R, spread, keep = z[name + "_R"], z[name + "_spread"], z[name + "_keep"]
    c = case(name)
    pairs, weights = _chosen(c, keep)
    assert (spread <= REFERENCE_SPREAD * np.abs(R).max()).all()
    return dict(keep=keep, pairs=pairs, weights=weights, g=slot_upstream(c, pairs, weights),
                directions=directions(c, SEAM_PROBES[name]), R=R, spread=spread)


if __name__ == "__main__":
    from concurrent.futures import ProcessPoolExecutor

    tasks = [(name, k) for name in FD_CASES for k in range(6 + len(SEAM_PROBES[name]))]
    with ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        results = dict(zip(tasks, pool.map(_probe, tasks)))
    out = {}
    for name in FD_CASES:
        ref = reference(name, _host_keep(name), [results[(name, k)] for k in range(6 + len(SEAM_PROBES[name]))])
        out.update({name + "_R": ref["R"], name + "_spread": ref["spread"], name + "_keep": ref["keep"]})
    os.makedirs(os.path.dirname(_GOLDEN), exist_ok=True)
    np.savez(_GOLDEN, **out)
