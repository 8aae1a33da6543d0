"""The reference of the tests of radfoam.cell_geometry_in_box_grad: difference quotients of the exact rational geometry of
the cells clipped to a box, by the method of tests/cell_geometry_grad_ref.py (its grid, steps, upstream scaling, probes
and bar) with the half-space machinery of tests/cell_box_ref.py (its ``_cell`` on the same plane list: the row in row
order, then the six walls).

For a cloud, a fixed box and upstreams (w, u) let  L = sum over the chosen cells of  w_a V_a + u_a . c_a,  V and c the
volume and centroid of cell(a) n box, an exact Fraction.  The clouds are rounded to multiples of 2^-16, the steps are
integer multiples of 2^-20, every perturbed cloud gets its own Qhull CSR, and with h = 2^-19

    D(h) = (L(p + h delta) - L(p - h delta)) / (2 h),   R = (4 D(h/2) - D(h)) / 3,   spread = |D(h/2) - D(h)|.

The bar of the tests is |<grad, delta> - R| <= spread per probe, under the condition -- on the reference alone -- that
spread <= 1e-3 max |R| over the case's probes.  The chosen cells must stay non-empty under every perturbation.

Nothing here shares code or numerics with radfoam_amd/csrc/rf_clip_box_grad.hpp.

R and spread of every case are recorded in tests/golden/cell_box_grad/fd.npz (``python -m tests.cell_box_grad_ref``
writes it).  The CPU test computes each reference afresh and requires the record to equal it bit for bit; the GPU tests
read the record (recorded()) and never run the rational code.
"""
from __future__ import annotations

import os
from fractions import Fraction

import numpy as np

from tests import cell_box_ref as X
from tests import cell_geometry_grad_ref as G
from tests.host_harness import clip_box_host as B

REFERENCE_SPREAD = G.REFERENCE_SPREAD

CUT16_BOX = (-5.0, -5.0, -5.0, 0.45, 5.0, 5.0)            # its +x wall cuts the ring face of sites 0 and 1
REDO_CUT_BOX = (-9.5, -9.5, -9.5, 2.45, 9.5, 9.5)        # its +x wall cuts the ring faces of pairs (2,3) and (200,201)
_HUB_CELLS = tuple(range(9))
_AXIS_SITES = tuple(s for pair in ((0, 1), (2, 3), (72, 73), (200, 201)) for s in pair)

# name -> (cloud, box, the cells of L (None: the non-empty cells of pick_cells), the single-coordinate seam probes)
FD_CASES = {
    "uniform400": ("uniform400", B.CASES["uniform400"][1], None, ()),
    "tight": ("uniform400", B.CASES["tight"][1], None, ()),
    "hub58": ("hub58", B.HUB_BOX, _HUB_CELLS, ((0, 0), (1, 1))),
    "hub59": ("hub59", B.HUB_BOX, _HUB_CELLS, ((0, 0), (1, 1))),
    "hub64": ("hub64", B.HUB_BOX, _HUB_CELLS, ((0, 0), (1, 1))),
    "hub65": ("hub65", B.HUB_BOX, _HUB_CELLS, ((0, 0), (1, 1))),
    "ring16_cut": ("ring16", CUT16_BOX, (0, 1), ((0, 2), (1, 0))),
    "ring17_cut": ("ring17", CUT16_BOX, (0, 1), ((0, 2), (1, 0))),
    "redo_spread_cut": ("redo_spread", REDO_CUT_BOX, _AXIS_SITES, ((2, 0), (73, 0), (200, 1))),
}
_CASES = {}
_REFS = {}
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cell_box_grad", "fd.npz")


def case(name: str) -> dict:
    """The cloud of case ``name`` on the 2^-16 grid with Qhull's CSR, its box, and the exact boxed geometry of the cells
    the case lists (``exact``, tests/cell_box_ref.exact_cells_in_box) with ``cells`` bool[N], the cells of L."""
    if name not in _CASES:
        from radfoam_amd import foam

        cl, box, cells, _ = FD_CASES[name]
        pts = G.rounded(B._CLOUDS[cl]())
        off, adj = foam.delaunay_csr(pts)
        box = np.array(box, dtype=np.float64)
        listed = B.pick_cells(pts, box) if cells is None else cells
        ex = X.exact_cells_in_box(pts, off, adj, box, listed)
        in_l = np.zeros(len(pts), dtype=bool)
        in_l[[a for a in listed if ex["volume"][a] > 0]] = True
        if cells is not None:
            assert in_l.sum() == len(cells)
        _CASES[name] = dict(points=pts, offsets=off, adjacency=adj, box=box, exact=ex, cells=in_l, name=name,
                            rows=np.repeat(np.arange(pts.shape[0]), np.diff(off.astype(np.int64))))
    return _CASES[name]


def upstreams(c: dict, cells: np.ndarray):
    """tests/cell_geometry_grad_ref.upstreams (w = r / s^2, u = r') with s from the exact boxed volumes"""
    return G.upstreams(dict(points=c["points"], exact=dict(volume_f=c["exact"]["volume_f"])), cells)


def exact_loss(points: np.ndarray, box: np.ndarray, w, u, cells) -> Fraction:
    """L of a cloud with its own Qhull CSR, every cell through cell_box_ref._cell on the forward's plane list"""
    from radfoam_amd import foam

    off, adj = foam.delaunay_csr(points)
    off, adj = off.astype(np.int64), adj.astype(np.int64)
    P = [tuple(Fraction(float(x)) for x in row) for row in points]
    lo, hi = [Fraction(float(x)) for x in box[:3]], [Fraction(float(x)) for x in box[3:]]
    allmin = np.minimum(points.min(0).astype(np.float64), box[:3])
    allmax = np.maximum(points.max(0).astype(np.float64), box[3:])
    reach = 2.0 * float(np.linalg.norm(allmax - allmin))
    total = Fraction(0)
    for a in np.nonzero(cells)[0]:
        planes = []
        for b in adj[off[a]:off[a + 1]]:
            d = tuple(P[b][q] - P[a][q] for q in range(3))
            planes.append((d, X._dot(d, d) / 2))
        for k in range(3):
            planes.append((tuple(Fraction(-int(q == k)) for q in range(3)), P[a][k] - lo[k]))
            planes.append((tuple(Fraction(int(q == k)) for q in range(3)), hi[k] - P[a][k]))
        volume, moment, _ = X._cell(planes, reach)
        assert volume > 0, f"cell {a} emptied under the perturbation"
        total += Fraction(float(w[a])) * volume
        total += sum(Fraction(float(u[a, k])) * (P[a][k] + moment[k] / volume) for k in range(3))
    return total


def quotient(points: np.ndarray, box: np.ndarray, delta: np.ndarray, w, u, cells):
    """(R, spread) for the integer direction delta i64[N,3]"""
    assert delta.dtype == np.int64
    out = []
    for h in (G.STEP, 0.5 * G.STEP):
        step = delta.astype(np.float64) * h
        plus, minus = (points.astype(np.float64) + step).astype(np.float32), (points.astype(np.float64) - step).astype(np.float32)
        assert np.array_equal(plus.astype(np.float64) - points, step) and np.array_equal(points - minus.astype(np.float64), step)
        diff = exact_loss(plus, box, w, u, cells) - exact_loss(minus, box, w, u, cells)
        out.append(float(diff / Fraction(2.0 * h)))
    d1, d2 = out
    return (4.0 * d2 - d1) / 3.0, abs(d2 - d1)


def reference(name: str) -> dict:
    """The difference-quotient reference of case ``name``: cells, w, u, the probes' directions, R and spread per probe.
    Computed once per process and never modified; asserts the condition on the reference."""
    if name not in _REFS:
        c = case(name)
        w, u = upstreams(c, c["cells"])
        dirs = G.directions(c, FD_CASES[name][3])
        got = [quotient(c["points"], c["box"], d, w, u, c["cells"]) for d in dirs]
        R, spread = np.array([g[0] for g in got]), np.array([g[1] for g in got])
        worst = spread.max() / np.abs(R).max()
        print(f"{name}: {c['cells'].sum()} cells in L, reference spread / max |R| = {worst:.3g} over {len(dirs)} probes "
              f"(max |R| = {np.abs(R).max():.4g})")
        assert worst <= REFERENCE_SPREAD
        _REFS[name] = dict(cells=c["cells"], w=w, u=u, directions=dirs, R=R, spread=spread, worst=worst)
    return _REFS[name]


def recorded(name: str) -> dict:
    """reference() as recorded in tests/golden: cells, w, u (they are scaled with the exact volumes, so they are recorded
    too), R and spread; the directions are derived again from the case's seed.  The rational code is not run."""
    with np.load(_GOLDEN) as z:
        cells, w, u, R, spread = (z[f"{name}_{k}"] for k in ("cells", "w", "u", "R", "spread"))
    assert (spread <= REFERENCE_SPREAD * np.abs(R).max()).all()
    n = len(cells)
    return dict(cells=cells, w=w, u=u, directions=G.directions(dict(points=np.empty((n, 3))), FD_CASES[name][3]), R=R,
                spread=spread)


def recorded_case(name: str) -> dict:
    """case() without the exact geometry: what the GPU tests need"""
    from radfoam_amd import foam

    cl, box, _, _ = FD_CASES[name]
    pts = G.rounded(B._CLOUDS[cl]())
    off, adj = foam.delaunay_csr(pts)
    return dict(points=pts, offsets=off, adjacency=adj, box=np.array(box, dtype=np.float64), name=name,
                rows=np.repeat(np.arange(pts.shape[0]), np.diff(off.astype(np.int64))))


def check_against_reference(name: str, ref: dict, grad: np.ndarray) -> float:
    """the bar: |<grad, delta> - R| <= spread on every probe; returns the worst |<grad, delta> - R| / spread"""
    got = np.array([(grad * d).sum() for d in ref["directions"]])
    miss = np.abs(got - ref["R"])
    for g, r, s, m in zip(got, ref["R"], ref["spread"], miss):
        print(f"{name}: <grad, delta> = {g:+.12e}, R = {r:+.12e}, |difference| = {m:.3g}, spread = {s:.3g}")
    worst = float((miss / ref["spread"]).max())
    print(f"{name}: spread / max |R| = {ref['spread'].max() / np.abs(ref['R']).max():.3g}, worst |<grad, delta> - R| / "
          f"spread = {worst:.3g}")
    assert np.isfinite(got).all() and (miss <= ref["spread"]).all()
    return worst


if __name__ == "__main__":
    import sys

    names = sys.argv[1:] or list(FD_CASES)
    out = {}
    if os.path.exists(_GOLDEN):
        with np.load(_GOLDEN) as z:
            out.update({k: z[k] for k in z.files})
    for name in names:
        ref = reference(name)
        out.update({f"{name}_{k}": ref[k] for k in ("cells", "w", "u", "R", "spread")})
    os.makedirs(os.path.dirname(_GOLDEN), exist_ok=True)
    np.savez(_GOLDEN, **out)
