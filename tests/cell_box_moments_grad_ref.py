"""The reference of the tests of radfoam.cell_moments_in_box_grad: difference quotients of the exact rational boxed moments
(tests/cell_box_moments_ref.exact_moments_in_box: ``site``, ``central``, ``volume``, ``first``), by the method of
tests/cell_box_grad_ref.py and with its cases: FD_CASES (the clouds on the 2^-16 grid, the boxes, the cells of L and the
single-coordinate seam probes), case() and recorded_case().

For a cloud, a fixed box and the four upstreams (A, B, w, u) -- all four at once -- let

    L = sum over the chosen cells of  <A_a, Q_a> + <B_a, C_a> + w_a V_a + u_a . c_a,

Q and C the site and central moment of cell(a) n box (six numbers each, the bracket their plain sum), V and c its volume and
centroid p_a + first / V: an exact Fraction.  Every perturbed cloud gets its own Qhull CSR, and with h = 2^-19

    D(h) = (L(p + h delta) - L(p - h delta)) / (2 h),   R = (4 D(h/2) - D(h)) / 3,   spread = |D(h/2) - D(h)|.

A and B are r / s_a^4 with s_a = V_a^(1/3) from the exact boxed volume (tests/cell_moments_grad_ref.upstreams), w and u
those of tests/cell_box_grad_ref.upstreams.  The probes of a case are PROBES random integer directions and its seam probes.
The chosen cells must stay non-empty under every perturbation.

The condition on the reference alone: spread <= 1e-3 max |R| per case.  The bar per probe:

    |<grad, delta> - R| <= max(spread, 1e-9 max |R| of the case).

The second term is the project's bar for doubles against an exact reference (clip_moments_host.BAR): the single-coordinate
probes agree between the two step sizes to 1e-13 .. 1e-12 of R, and the floor keeps a probe from asking more than double
arithmetic has.

Nothing here shares code or numerics with radfoam_amd/csrc/rf_clip_box_moments_grad.hpp.

A probe costs four exact evaluations, so R and spread of every probe are recorded in
tests/golden/cell_box_moments_grad/fd.npz (``python -m tests.cell_box_moments_grad_ref`` writes it, one process per
probe).  The CPU test computes one random probe and every seam probe of every case afresh and requires the record to equal
them bit for bit; the GPU tests read the record (recorded()) and never run the rational code.
"""
from __future__ import annotations

import os
from fractions import Fraction

import numpy as np

from tests import cell_box_grad_ref as BR
from tests import cell_box_moments_ref as M
from tests import cell_geometry_grad_ref as G
from tests import cell_moments_grad_ref as MG

STEP = G.STEP
REFERENCE_SPREAD = 1e-3   # a reference whose two step sizes disagree by more than this (of max |R|) is not a reference
FLOOR = 1e-9              # of max |R| of the case: clip_moments_host.BAR, doubles against an exact reference
PROBES = 2                # random directions per case, before the seam probes

FD_CASES = BR.FD_CASES
case = BR.case
recorded_case = BR.recorded_case
_PROBES = {}
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cell_box_moments_grad", "fd.npz")


def upstreams(c: dict, cells: np.ndarray):
    """(A f64[N,6], B f64[N,6], w f64[N], u f64[N,3]), zero outside ``cells``, scaled with the exact boxed volumes"""
    A, B = MG.upstreams(dict(points=c["points"], exact=dict(volume_f=c["exact"]["volume_f"])), cells)
    w, u = BR.upstreams(c, cells)
    return A, B, w, u


def exact_loss(points: np.ndarray, box: np.ndarray, A, B, w, u, cells) -> Fraction:
    """L of a cloud with its own Qhull CSR"""
    from radfoam_amd import foam

    off, adj = foam.delaunay_csr(points)
    pick = np.nonzero(cells)[0]
    ex = M.exact_moments_in_box(points, off, adj, box, pick)
    M._CACHE.clear()                                           # one of many perturbed clouds: not worth keeping
    total = Fraction(0)
    for a in pick:
        volume = ex["volume"][a]
        assert volume > 0, f"cell {a} emptied under the perturbation"
        total += sum(Fraction(float(A[a, k])) * ex["site"][a][k] for k in range(6))
        total += sum(Fraction(float(B[a, k])) * ex["central"][a][k] for k in range(6))
        total += Fraction(float(w[a])) * volume
        total += sum(Fraction(float(u[a, k])) * (Fraction(float(points[a, k])) + ex["first"][a][k] / volume)
                     for k in range(3))
    return total


def quotient(points: np.ndarray, box: np.ndarray, delta: np.ndarray, A, B, w, u, cells):
    """(R, spread) for the integer direction delta i64[N,3]"""
    assert delta.dtype == np.int64
    out = []
    for h in (STEP, 0.5 * STEP):
        step = delta.astype(np.float64) * h
        plus, minus = (points.astype(np.float64) + step).astype(np.float32), (points.astype(np.float64) - step).astype(np.float32)
        assert np.array_equal(plus.astype(np.float64) - points, step) and np.array_equal(points - minus.astype(np.float64), step)
        diff = exact_loss(plus, box, A, B, w, u, cells) - exact_loss(minus, box, A, B, w, u, cells)
        out.append(float(diff / Fraction(2.0 * h)))
    d1, d2 = out
    return (4.0 * d2 - d1) / 3.0, abs(d2 - d1)


def directions(n: int, name: str):
    return G.directions(dict(points=np.empty((n, 3))), FD_CASES[name][3], count=PROBES)


def probe(name: str, index: int):
    """(R, spread) of probe ``index`` of case ``name``, computed once per process"""
    key = (name, index)
    if key not in _PROBES:
        c = case(name)
        _PROBES[key] = quotient(c["points"], c["box"], directions(len(c["points"]), name)[index],
                                *upstreams(c, c["cells"]), c["cells"])
    return _PROBES[key]


def recorded(name: str) -> dict:
    """The record in tests/golden: cells, A, B, w, u (they are scaled with the exact volumes, so they are recorded too), R
    and spread per probe; the directions are derived again from the case's seed.  Asserts the condition on the reference.
    The rational code is not run."""
    with np.load(_GOLDEN) as z:
        cells, A, B, w, u, R, spread = (z[f"{name}_{k}"] for k in ("cells", "A", "B", "w", "u", "R", "spread"))
    dirs = directions(len(cells), name)
    assert len(dirs) == len(R) == len(spread) == PROBES + len(FD_CASES[name][3])
    assert (spread <= REFERENCE_SPREAD * np.abs(R).max()).all()
    return dict(cells=cells, A=A, B=B, w=w, u=u, directions=dirs, R=R, spread=spread,
                worst=spread.max() / np.abs(R).max())


def check_against_reference(name: str, ref: dict, grad: np.ndarray) -> float:
    """the bar: |<grad, delta> - R| <= max(spread, 1e-9 max |R|) on every probe; prints each figure and which probes
    needed the floor; returns the worst |difference| / spread"""
    got = np.array([(grad * d).sum() for d in ref["directions"]])
    miss = np.abs(got - ref["R"])
    floor = FLOOR * np.abs(ref["R"]).max()
    for i, (g, r, s, m) in enumerate(zip(got, ref["R"], ref["spread"], miss)):
        print(f"{name}: probe {i}: <grad, delta> = {g:+.12e}, R = {r:+.12e}, |difference| = {m:.3g}, spread = {s:.3g}, "
              f"floor = {floor:.3g}{' (needed the floor)' if s < m <= floor else ''}")
    worst = float((miss / ref["spread"]).max())
    print(f"{name}: spread / max |R| = {ref['spread'].max() / np.abs(ref['R']).max():.3g}, worst |<grad, delta> - R| / "
          f"spread = {worst:.3g}, worst |<grad, delta> - R| / max |R| = {miss.max() / np.abs(ref['R']).max():.3g}")
    assert np.isfinite(got).all() and (miss <= np.maximum(ref["spread"], floor)).all()
    return worst


def _job(job):
    name, index = job
    c = case(name)
    return name, index, c["cells"], upstreams(c, c["cells"]), probe(name, index)


if __name__ == "__main__":
    import sys
    from concurrent.futures import ProcessPoolExecutor

    names = sys.argv[1:] or list(FD_CASES)
    jobs = [(name, i) for name in names for i in range(PROBES + len(FD_CASES[name][3]))]
    out = {}
    if os.path.exists(_GOLDEN):
        with np.load(_GOLDEN) as z:
            out.update({k: z[k] for k in z.files})
    got = {}
    with ProcessPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1)) as pool:
        for name, index, cells, (A, B, w, u), (R, spread) in pool.map(_job, jobs):
            out.update({f"{name}_cells": cells, f"{name}_A": A, f"{name}_B": B, f"{name}_w": w, f"{name}_u": u})
            got.setdefault(name, {})[index] = (R, spread)
    for name in names:
        out[f"{name}_R"] = np.array([got[name][i][0] for i in range(len(got[name]))])
        out[f"{name}_spread"] = np.array([got[name][i][1] for i in range(len(got[name]))])
        worst = out[f"{name}_spread"].max() / np.abs(out[f"{name}_R"]).max()
        print(f"{name}: {int(out[f'{name}_cells'].sum())} cells, reference spread / max |R| = {worst:.3g} over "
              f"{len(out[f'{name}_R'])} probes (max |R| = {np.abs(out[f'{name}_R']).max():.4g})")
        assert worst <= REFERENCE_SPREAD
    os.makedirs(os.path.dirname(_GOLDEN), exist_ok=True)
    np.savez_compressed(_GOLDEN, **out)
