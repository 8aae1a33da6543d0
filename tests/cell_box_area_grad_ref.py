"""The reference of the tests of radfoam.face_area_in_box_grad: difference quotients of the exact face and wall areas of
the cells clipped to a box, by the method of tests/cell_box_grad_ref.py (its cases FD_CASES: the clouds on the 2^-16
grid, the boxes, the cells and the seam probes; h = 2^-19, R = (4 D(h/2) - D(h)) / 3, spread = |D(h/2) - D(h)|, a Qhull
CSR per perturbed cloud) and of tests/face_area_grad_ref.py (areas as Fractions through math.isqrt).

tests/cell_box_ref._cell returns areas as floats, which is useless for a quotient, so this file runs its own face loop over
the same plane list (the row in row order, then the six walls) with that file's _clip, _dot and _cross: the face on plane
i is cut in the plane's rational basis u = n x e, v = n x u, Q is its area in (s,t), and

    area^2 = Q^2 |u|^4 |n|^2,    area = Q |u|^2 sqrt(|n|^2),

sqrt(p / q) = isqrt(p q 2^512) / (q 2^256), rounded down: relative 2^-256, far below the spread.  So
L = sum g_s A_s + sum gw_{a,w} W_{a,w}  is a Fraction.  It runs over the slots (a -> b) and walls (a, w) of the case's
cells whose exact base area is positive and that the kept mask keeps (kept(): all of them, see there), each with a weight
of its own: g_s = r / cbrt(min(V_a, V_b)) (V_b where the exact boxed volume of b is known and positive, else V_a alone)
and gw_{a,w} = r / cbrt(V_a), r uniform in [-1,1] from a fixed seed, one draw per slot and per wall of the cloud.  A slot
the perturbation flips away has area 0; one it flips in has no weight.  The areas are C^1 across flips, so the quotients
converge whether or not a flip falls in the step.

The bar of the tests is |<grad, delta> - R| <= spread per probe, under the condition -- on the reference alone -- that
spread <= 1e-3 max |R| over the case's probes (REFERENCE_SPREAD).

Nothing here shares code or numerics with radfoam_amd/csrc/rf_clip_box_area_grad.hpp.

The kept masks, the weights, R and spread of every case are recorded in tests/golden/cell_box_area_grad/fd.npz (``python -m
tests.cell_box_area_grad_ref`` writes it, one process per probe).  The CPU test computes each reference afresh and
requires the record to equal it bit for bit; the GPU tests read the record (recorded()) and never run the rational code.
"""
from __future__ import annotations

import math
import os
from fractions import Fraction

import numpy as np

from tests import cell_box_grad_ref as BR
from tests import cell_geometry_grad_ref as G
from tests.cell_box_ref import _clip, _cross, _dot

FD_CASES, REFERENCE_SPREAD, STEP = BR.FD_CASES, BR.REFERENCE_SPREAD, G.STEP
ROOT_BITS = 256
KEEP_SHARE = 0.9          # of the positive-area slots and of the positive-area walls of a case's cells
_REFS = {}
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cell_box_area_grad", "fd.npz")

case, recorded_case = BR.case, BR.recorded_case


def _root(x: Fraction) -> Fraction:
    p, q = x.numerator, x.denominator
    return Fraction(math.isqrt((p * q) << (2 * ROOT_BITS)), q << ROOT_BITS)


def _area(planes, i: int, reach: float) -> Fraction:
    """the exact area of the face on plane i of the list, the construction of cell_box_ref._cell"""
    n, h = planes[i]
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
    Q2 = Fraction(0)
    for a in range(1, len(poly) - 1):
        ps, pt = poly[a][0] - poly[0][0], poly[a][1] - poly[0][1]
        qs, qt = poly[a + 1][0] - poly[0][0], poly[a + 1][1] - poly[0][1]
        Q2 += ps * qt - pt * qs
    assert Q2 >= 0
    return Q2 * uu * _root(nn) / 2 if Q2 else Fraction(0)


def exact_areas(points: np.ndarray, box: np.ndarray, wanted: dict) -> dict:
    """wanted: {a: (neighbours, walls)}.  Returns {a: ({b: area}, {w: area})} as Fractions from the cloud's own Qhull CSR;
    a neighbour that is not in a's row has area 0."""
    from radfoam_amd import foam

    off, adj = foam.delaunay_csr(points)
    off, adj = off.astype(np.int64), adj.astype(np.int64)
    P = [tuple(Fraction(float(x)) for x in row) for row in points]
    lo, hi = [Fraction(float(x)) for x in box[:3]], [Fraction(float(x)) for x in box[3:]]
    allmin = np.minimum(points.min(0).astype(np.float64), box[:3])
    allmax = np.maximum(points.max(0).astype(np.float64), box[3:])
    reach = 2.0 * float(np.linalg.norm(allmax - allmin))
    out = {}
    for a, (nbrs, walls) in wanted.items():
        row = adj[off[a]:off[a + 1]].tolist()
        planes = []
        for b in row:
            d = tuple(P[b][q] - P[a][q] for q in range(3))
            planes.append((d, _dot(d, d) / 2))
        for k in range(3):
            planes.append((tuple(Fraction(-int(q == k)) for q in range(3)), P[a][k] - lo[k]))
            planes.append((tuple(Fraction(int(q == k)) for q in range(3)), hi[k] - P[a][k]))
        at = {b: i for i, b in enumerate(row)}
        out[a] = ({b: (_area(planes, at[b], reach) if b in at else Fraction(0)) for b in nbrs},
                  {w: _area(planes, len(row) + w, reach) for w in walls})
    return out


def base(name: str) -> dict:
    """The exact areas of every slot and wall of the case's cells on the unperturbed cloud (floats of the Fractions;
    positive means positive), and the draws: slot_area f64[E] and wall_area f64[N,6] (NaN outside the case's cells),
    g f64[E] and gw f64[N,6] for every slot and wall of positive area of the case's cells, zero elsewhere."""
    c = case(name)
    n, e = len(c["points"]), len(c["adjacency"])
    off, adj = c["offsets"].astype(np.int64), c["adjacency"].astype(np.int64)
    cells = np.nonzero(c["cells"])[0].tolist()
    areas = exact_areas(c["points"], c["box"], {a: (adj[off[a]:off[a + 1]].tolist(), range(6)) for a in cells})
    slot_area, wall_area = np.full(e, np.nan), np.full((n, 6), np.nan)
    positive_slot, positive_wall = np.zeros(e, dtype=bool), np.zeros((n, 6), dtype=bool)
    for a in cells:
        for k in range(off[a], off[a + 1]):
            x = areas[a][0][int(adj[k])]
            slot_area[k], positive_slot[k] = float(x), x > 0
        for w in range(6):
            x = areas[a][1][w]
            wall_area[a, w], positive_wall[a, w] = float(x), x > 0
    vol = c["exact"]["volume_f"]                                  # NaN where the exact reference did not work
    va, vb = vol[c["rows"]], vol[adj]
    size = np.cbrt(np.where(vb > 0, np.fmin(va, vb), va))
    rng = np.random.default_rng(0)
    r, rw = rng.uniform(-1.0, 1.0, e), rng.uniform(-1.0, 1.0, (n, 6))
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.where(positive_slot, r / size, 0.0)
        gw = np.where(positive_wall, rw / np.cbrt(vol)[:, None], 0.0)
    assert np.isfinite(g).all() and np.isfinite(gw).all()
    return dict(slot_area=slot_area, wall_area=wall_area, positive_slot=positive_slot, positive_wall=positive_wall, g=g,
                gw=gw)


def kept(name: str, b: dict):
    """(keep_slot bool[E], keep_wall bool[N,6]): the slots and walls of L.  Every slot and wall of positive exact base
    area of the case's cells is kept: all nine cases meet the condition on the reference that way (spread / max |R| is
    between 5.9e-9 and 9.1e-6; DESIGN.md has the table), so no rule drops anything.  Asserts what the tests
    rely on: at least KEEP_SHARE of each, and at least one wall and one wall-cut face (a kept slot of a cell with a
    kept wall; the cases' own seams are asserted in the CPU test)."""
    keep_slot, keep_wall = b["positive_slot"].copy(), b["positive_wall"].copy()
    assert keep_slot.sum() >= KEEP_SHARE * b["positive_slot"].sum() > 0
    assert keep_wall.sum() >= KEEP_SHARE * b["positive_wall"].sum() > 0
    return keep_slot, keep_wall


def _wanted(c: dict, g: np.ndarray, gw: np.ndarray) -> dict:
    off, adj = c["offsets"].astype(np.int64), c["adjacency"].astype(np.int64)
    out = {}
    for a in np.nonzero(c["cells"])[0].tolist():
        slots = [k for k in range(off[a], off[a + 1]) if g[k] != 0.0]
        walls = [w for w in range(6) if gw[a, w] != 0.0]
        if slots or walls:
            out[a] = ([(int(adj[k]), float(g[k])) for k in slots], [(w, float(gw[a, w])) for w in walls])
    return out


def exact_loss(points: np.ndarray, box: np.ndarray, wanted: dict) -> Fraction:
    areas = exact_areas(points, box, {a: ([b for b, _ in s], [w for w, _ in ws]) for a, (s, ws) in wanted.items()})
    total = Fraction(0)
    for a, (slots, walls) in wanted.items():
        total += sum(Fraction(x) * areas[a][0][b] for b, x in slots)
        total += sum(Fraction(x) * areas[a][1][w] for w, x in walls)
    return total


def quotient(points: np.ndarray, box: np.ndarray, delta: np.ndarray, wanted: dict):
    """(R, spread) for the integer direction delta i64[N,3]"""
    assert delta.dtype == np.int64
    out = []
    for h in (STEP, 0.5 * STEP):
        step = delta.astype(np.float64) * h
        plus, minus = (points.astype(np.float64) + step).astype(np.float32), (points.astype(np.float64) - step).astype(np.float32)
        assert np.array_equal(plus.astype(np.float64) - points, step) and np.array_equal(points - minus.astype(np.float64), step)
        diff = exact_loss(plus, box, wanted) - exact_loss(minus, box, wanted)
        out.append(float(diff / Fraction(2.0 * h)))
    d1, d2 = out
    return (4.0 * d2 - d1) / 3.0, abs(d2 - d1)


def _weights(name: str):
    c = case(name)
    b = base(name)
    keep_slot, keep_wall = kept(name, b)
    return c, keep_slot, keep_wall, np.where(keep_slot, b["g"], 0.0), np.where(keep_wall, b["gw"], 0.0)


def _probe(task):
    name, k = task
    c, _, _, g, gw = _weights(name)
    return quotient(c["points"], c["box"], G.directions(c, FD_CASES[name][3])[k], _wanted(c, g, gw))


def probes(name: str) -> int:
    return 6 + len(FD_CASES[name][3])


def reference(name: str, got=None) -> dict:
    """The difference-quotient reference of case ``name``: the kept masks, g and gw, the probes' directions, R and spread
    per probe.  Computed once per process and never modified; asserts the condition on the reference."""
    if name not in _REFS:
        c, keep_slot, keep_wall, g, gw = _weights(name)
        dirs = G.directions(c, FD_CASES[name][3])
        if got is None:
            wanted = _wanted(c, g, gw)
            got = [quotient(c["points"], c["box"], d, wanted) for d in dirs]
        R, spread = np.array([x[0] for x in got]), np.array([x[1] for x in got])
        worst = spread.max() / np.abs(R).max()
        print(f"{name}: {keep_slot.sum()} slots and {keep_wall.sum()} walls in L, reference spread / max |R| = {worst:.3g} "
              f"over {len(dirs)} probes (max |R| = {np.abs(R).max():.4g})")
        assert worst <= REFERENCE_SPREAD
        _REFS[name] = dict(keep_slot=keep_slot, keep_wall=keep_wall, g=g, gw=gw, directions=dirs, R=R, spread=spread,
                           worst=worst)
    return _REFS[name]


_KEYS = ("keep_slot", "keep_wall", "g", "gw", "R", "spread")


def recorded(name: str) -> dict:
    """reference() as recorded in tests/golden; the directions are derived again from the case's seed.  The rational code
    is not run."""
    with np.load(_GOLDEN) as z:
        out = {k: z[f"{name}_{k}"] for k in _KEYS}
    assert (out["spread"] <= REFERENCE_SPREAD * np.abs(out["R"]).max()).all()
    n = out["gw"].shape[0]
    out["directions"] = G.directions(dict(points=np.empty((n, 3))), FD_CASES[name][3])
    return out


def check_against_reference(name: str, ref: dict, grad: np.ndarray) -> float:
    return BR.check_against_reference(name, ref, grad)


if __name__ == "__main__":
    import sys
    from concurrent.futures import ProcessPoolExecutor

    names = sys.argv[1:] or list(FD_CASES)
    out = {}
    if os.path.exists(_GOLDEN):
        with np.load(_GOLDEN) as z:
            out.update({k: z[k] for k in z.files})
    tasks = [(name, k) for name in names for k in range(probes(name))]
    with ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        results = dict(zip(tasks, pool.map(_probe, tasks)))
    for name in names:
        ref = reference(name, [results[(name, k)] for k in range(probes(name))])
        out.update({f"{name}_{k}": ref[k] for k in _KEYS})
    os.makedirs(os.path.dirname(_GOLDEN), exist_ok=True)
    np.savez_compressed(_GOLDEN, **out)
