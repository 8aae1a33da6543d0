"""The reference of the cell-moment gradient tests: difference quotients of the exact rational second moments
(tests/cell_moments_ref.exact_moments), with their own error measured, by the scheme of tests/cell_geometry_grad_ref.py
and with that module's pieces: case() (the clouds on the 2^-16 grid), directions(), SEAM_PROBES and STEP = 2^-19.

For a cloud and upstreams (A, B), six numbers per cell each, let  L = sum over the chosen bounded cells of
<A_a, Q_a> + <B_a, C_a> = sum_k A_a[k] site_moment[a][k] + B_a[k] central_moment[a][k],  an exact Fraction.  For an
integer direction delta, with h = 2^-19,

    D(h) = (L(p + h delta) - L(p - h delta)) / (2 h),   R = (4 D(h/2) - D(h)) / 3,   spread = |D(h/2) - D(h)|.

R is the reference value of <grad, delta> and the spread its uncertainty: the bar of the tests is |<grad, delta> - R| <=
spread, under the condition -- on the reference alone -- that spread <= 1e-3 max |R| over the case's probes.  Q and C are
C^1 across Delaunay flips (a face that appears has zero area and the integrand is bounded), so the quotients converge
whether or not a flip falls inside the step.

The probes of a case are PROBES random directions and the single-coordinate probes of SEAM_PROBES.  L runs over the cells
the host forward calls bounded; on uniform400 over every eighth of them (UNIFORM_STRIDE; 44 cells), since one exact
evaluation of all 352 costs 40 s: their neighbours' rows still receive gradient, which is the point of the gather.

Nothing here shares code or numerics with radfoam_amd/csrc/rf_clip_moments_grad.hpp.

A probe costs four exact evaluations (10 to 15 s each), so R and spread of every probe are recorded in
tests/golden/cell_moments_grad/fd.npz (``python -m tests.cell_moments_grad_ref`` writes it, one process per probe).  The
CPU test computes one random probe and every seam probe of every case afresh and requires the record to equal them bit for
bit; the GPU tests read the record (recorded()).
"""
from __future__ import annotations

import os
from fractions import Fraction

import numpy as np

from tests import cell_geometry_grad_ref as G
from tests import cell_geometry_ref as X
from tests import cell_moments_ref as M

STEP = G.STEP
REFERENCE_SPREAD = 1e-3   # a reference whose two step sizes disagree by more than this (of max |R|) is not a reference
PROBES = 2                # random directions per case, before the seam probes
UNIFORM_STRIDE = 8        # uniform400: L over every eighth bounded cell

FD_CASES = G.FD_CASES
SEAM_PROBES = G.SEAM_PROBES
case = G.case
_PROBES = {}
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cell_moments_grad", "fd.npz")


def loss_cells(name: str, bounded: np.ndarray) -> np.ndarray:
    """bool[N]: the cells L sums over, from the host forward's bounded cells"""
    cells = np.asarray(bounded, dtype=bool).copy()
    if name == "uniform400":
        keep = np.nonzero(cells)[0][::UNIFORM_STRIDE]
        cells[:] = False
        cells[keep] = True
    return cells


def upstreams(c: dict, cells: np.ndarray, seed: int = 0):
    """(A f64[N,6], B f64[N,6]): r / s_a^4 with r uniform in [-1,1] and s_a = V_a^(1/3), so that every cell's own term of
    its row is O(1); zero outside ``cells`` (bool[N])."""
    rng = np.random.default_rng(seed)
    n = len(c["points"])
    size = np.cbrt(np.where(cells, c["exact"]["volume_f"], 1.0))[:, None]
    A = np.where(cells[:, None], rng.uniform(-1.0, 1.0, (n, 6)) / size ** 4, 0.0)
    B = np.where(cells[:, None], rng.uniform(-1.0, 1.0, (n, 6)) / size ** 4, 0.0)
    return A, B


def exact_loss(points: np.ndarray, A: np.ndarray, B: np.ndarray, cells: np.ndarray) -> Fraction:
    pick = np.nonzero(cells)[0]
    ex = M.exact_moments(points, cells=pick)
    M._CACHE.clear()                                           # one of many perturbed clouds: not worth keeping
    X._CACHE.pop((points.shape, points.tobytes()), None)
    assert ex["done"][pick].all(), "a cell opened under the perturbation"
    total = Fraction(0)
    for a in pick:
        total += sum(Fraction(float(A[a, k])) * ex["site"][a][k] for k in range(6))
        total += sum(Fraction(float(B[a, k])) * ex["central"][a][k] for k in range(6))
    return total


def quotient(points: np.ndarray, delta: np.ndarray, A, B, cells):
    """(R, spread) for the integer direction delta i64[N,3]"""
    assert delta.dtype == np.int64
    out = []
    for h in (STEP, 0.5 * STEP):
        step = delta.astype(np.float64) * h
        plus, minus = (points.astype(np.float64) + step).astype(np.float32), (points.astype(np.float64) - step).astype(np.float32)
        assert np.array_equal(plus.astype(np.float64) - points, step) and np.array_equal(points - minus.astype(np.float64), step)
        diff = exact_loss(plus, A, B, cells) - exact_loss(minus, A, B, cells)
        out.append(float(diff / Fraction(2.0 * h)))
    d1, d2 = out
    return (4.0 * d2 - d1) / 3.0, abs(d2 - d1)


def directions(c: dict, name: str):
    return G.directions(c, SEAM_PROBES[name], count=PROBES)


def probe(name: str, cells: np.ndarray, index: int):
    """(R, spread) of probe ``index`` of case ``name`` for L over ``cells``, computed once per process"""
    key = (name, cells.tobytes(), index)
    if key not in _PROBES:
        c = case(name)
        assert not c["exact"]["open"][cells].any()
        A, B = upstreams(c, cells)
        _PROBES[key] = quotient(c["points"], directions(c, name)[index], A, B, cells)
    return _PROBES[key]


def recorded(name: str) -> dict:
    """The record in tests/golden: cells, A, B, directions, R, spread (A, B and the directions are derived again from the
    recorded cells; they are functions of the case and its seeds).  Asserts the condition on the reference."""
    with np.load(_GOLDEN) as z:
        cells, R, spread = z[name + "_cells"], z[name + "_R"], z[name + "_spread"]
    c = case(name)
    assert not c["exact"]["open"][cells].any()
    A, B = upstreams(c, cells)
    dirs = directions(c, name)
    assert len(dirs) == len(R) == len(spread) == PROBES + len(SEAM_PROBES[name])
    assert (spread <= REFERENCE_SPREAD * np.abs(R).max()).all()
    return dict(cells=cells, A=A, B=B, directions=dirs, R=R, spread=spread, worst=spread.max() / np.abs(R).max())


def check_against_reference(name: str, ref: dict, grad: np.ndarray) -> float:
    """the bar: |<grad, delta> - R| <= spread on every probe; returns the worst |difference| / spread"""
    got = np.array([(grad * d).sum() for d in ref["directions"]])
    miss = np.abs(got - ref["R"])
    for g, r, s, m in zip(got, ref["R"], ref["spread"], miss):
        print(f"{name}: <grad, delta> = {g:+.12e}, R = {r:+.12e}, |difference| = {m:.3g}, spread = {s:.3g}")
    assert np.isfinite(got).all() and (miss <= ref["spread"]).all()
    return float((miss / ref["spread"]).max())


def _job(job):
    from tests.host_harness import clip_grad_host as HG

    name, index = job
    cells = loss_cells(name, HG.host_forward(("rounded", name), case(name))["bounded"])
    return name, index, cells, probe(name, cells, index)


if __name__ == "__main__":
    from concurrent.futures import ProcessPoolExecutor

    jobs = [(name, i) for name in FD_CASES for i in range(PROBES + len(SEAM_PROBES[name]))]
    out = {}
    with ProcessPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1)) as pool:
        for name, index, cells, (R, spread) in pool.map(_job, jobs):
            out[name + "_cells"] = cells
            out.setdefault(name + "_R", {})[index] = R
            out.setdefault(name + "_spread", {})[index] = spread
    for name in FD_CASES:
        for key in (name + "_R", name + "_spread"):
            out[key] = np.array([out[key][i] for i in range(len(out[key]))])
        worst = out[name + "_spread"].max() / np.abs(out[name + "_R"]).max()
        print(f"{name}: {int(out[name + '_cells'].sum())} cells, reference spread / max |R| = {worst:.3g} over "
              f"{len(out[name + '_R'])} probes (max |R| = {np.abs(out[name + '_R']).max():.4g})")
        assert worst <= REFERENCE_SPREAD
    os.makedirs(os.path.dirname(_GOLDEN), exist_ok=True)
    np.savez(_GOLDEN, **out)
