"""Point gradients of the cells' second moments, the part that runs without a GPU: radfoam_amd/csrc/
rf_clip_moments_grad.hpp compiled for the host (tests/host_harness/clip_moments_grad_host) against difference quotients of
the exact rational moments (tests/cell_moments_grad_ref.py), the fan's third-order sums against exact polygon integrals,
the closed form of the centroidal-Voronoi energy, the translation and scaling identities, and the degenerate inputs.
tests/test_gpu_cell_moments_grad.py holds the device to the same bars.

L sums over cells the host forward calls bounded (tests/cell_moments_grad_ref.loss_cells); the upstreams of the reference
are zero elsewhere.

Measured on the host (spread / max |R| of the reference, then the worst |<grad, delta> - R| / spread over the probes):
  uniform400 4.1e-7 4.8e-7, hub64 3.6e-10 4.8e-4, hub65 1.1e-9 2.6e-3, ring16 3.5e-9 2.4e-2, ring17 3.0e-9 5.8e-3,
  redo_spread 2.3e-8 2.8e-3 (the worst ratios are on the single-coordinate probes, whose spread is 1e-13 .. 1e-11)."""
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import cell_moments_grad_ref as MG
from tests.host_harness import clip_grad_host as HG
from tests.host_harness import clip_host as H
from tests.host_harness import clip_moments_grad_host as HMG


def _rounded(name):
    """(case on the 2^-16 grid, host forward)"""
    c = MG.case(name)
    return c, HG.host_forward(("rounded", name), c)


def _host_grad(c, geo, gq, gc, cap=256):
    got = HMG.cell_moments_grad(c["points"], c["adjacency"], c["offsets"], geo, gq, gc, cap=cap)
    assert got["bad"] == 0
    return got["grad"]


def test_sources_are_built_but_not_part_of_the_source_hash():
    from radfoam_amd import _lib, build

    names = lambda paths: {os.path.basename(p) for p in paths}
    assert "rf_cell_moments_grad.hip" in names(build.EXTRA_SOURCES)
    assert {"rf_clip_moments_grad.hpp", "radfoam_hip_moments_grad.h"} <= names(build.EXTRA_HEADERS)
    assert not names(build.SOURCES + build.HEADERS) & names(build.EXTRA_SOURCES + build.EXTRA_HEADERS)
    lib = _lib.load()
    for name in ("rf_cell_moments_grad", "rf_cell_moments_grad_workspace_bytes"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.rf_cell_moments_grad_workspace_bytes(1000) >= 1000
    none = [None] * 7
    assert lib.rf_cell_moments_grad(None, 0, None, None, 0, None, *none, None, 0, None) == 0      # nothing to do
    assert lib.rf_cell_moments_grad(None, 5, None, None, 0, None, *none, None, 0, None) == -1
    assert "null pointer" in _lib.last_error()
    dummy = np.zeros(64).ctypes.data
    assert lib.rf_cell_moments_grad(dummy, 5, dummy, dummy, 4, dummy, *([dummy] * 7), dummy, 2, None) == -2
    assert "workspace" in _lib.last_error()


def test_public_names_and_input_checks_without_a_device():
    import torch

    import radfoam
    import radfoam_amd

    for name in ("cell_moments_grad", "differentiable_cell_moments"):
        assert name in radfoam.__all__ and name in radfoam_amd.__all__ and callable(getattr(radfoam, name))
    pts = torch.zeros(10, 3)
    adj, off = torch.zeros(5, dtype=torch.uint32), torch.zeros(11, dtype=torch.uint32)
    with pytest.raises(RuntimeError, match="points must be a float32 CUDA tensor"):
        radfoam.differentiable_cell_moments(pts, adj, off)
    with pytest.raises(RuntimeError, match="points must be a float32 CUDA tensor"):
        radfoam.cell_moments_grad(pts, adj, off, None)
    assert "differentiable_cell_moments" in radfoam.cell_moments.__doc__


@pytest.mark.parametrize("name", MG.FD_CASES)
def test_gradient_matches_difference_quotients_of_the_exact_moments(name):
    """One random probe and every seam probe are computed afresh and the record must equal them bit for bit; the bar is
    then held on every recorded probe."""
    c, geo = _rounded(name)
    cells = MG.loss_cells(name, geo["bounded"])
    assert not c["exact"]["open"][cells].any()
    if name == "uniform400":
        assert 40 <= cells.sum() <= 48
    else:                          # the seam cells are in L
        assert cells.sum() >= 0.9 * (~c["exact"]["open"]).sum() and cells[[s for s, _ in MG.SEAM_PROBES[name]]].all()
    rec = MG.recorded(name)
    assert np.array_equal(rec["cells"], cells)
    for index in [0] + list(range(MG.PROBES, len(rec["R"]))):
        R, spread = MG.probe(name, cells, index)
        assert R == rec["R"][index] and spread == rec["spread"][index]
    print(f"{name}: reference spread / max |R| = {rec['worst']:.3g} over {len(rec['R'])} probes")
    grad = _host_grad(c, geo, rec["A"], rec["B"])
    worst = MG.check_against_reference(name, rec, grad)
    print(f"{name}: worst |<grad, delta> - R| / spread = {worst:.3g}")
    # the same through a capacity that just fits, and a capacity below the face is reported, never a wrong number
    if name in ("ring16", "ring17"):
        k = int(name[4:])
        fits = HMG.cell_moments_grad(c["points"], c["adjacency"], c["offsets"], geo, rec["A"], rec["B"], cap=k)
        assert (fits["status"][:2] == 0).all() and np.array_equal(fits["grad"][:2], grad[:2])
        small = HMG.cell_moments_grad(c["points"], c["adjacency"], c["offsets"], geo, rec["A"], rec["B"], cap=k - 1)
        assert (small["status"][:2] == 1).all() and np.isnan(small["grad"][:2]).all()
        ok = small["status"] == 0
        assert np.array_equal(small["grad"][ok], grad[ok])


# ---- the fan's third-order sums ---------------------------------------------------------------------------------------

def _poly_mul(p, q):
    out = [Fraction(0)] * (len(p) + len(q) - 1)
    for i, a in enumerate(p):
        for j, b in enumerate(q):
            out[i + j] += a * b
    return out


def _exact_monomial(xs, ys, i, j):
    """int x^i y^j dA over the polygon, exactly, by Green's theorem: (1 / (i + 1)) sum over the edges of
    int_0^1 x(tau)^(i+1) y(tau)^j y'(tau) dtau with x, y linear in tau (no triangles, no fan)"""
    total = Fraction(0)
    for k in range(len(xs)):
        x0, y0, x1, y1 = xs[k], ys[k], xs[(k + 1) % len(xs)], ys[(k + 1) % len(xs)]
        poly = [Fraction(1)]
        for _ in range(i + 1):
            poly = _poly_mul(poly, [x0, x1 - x0])
        for _ in range(j):
            poly = _poly_mul(poly, [y0, y1 - y0])
        total += (y1 - y0) * sum(coef / (d + 1) for d, coef in enumerate(poly))
    return total / (i + 1)


def _polygons():
    rng = np.random.default_rng(7)
    ang = np.sort(rng.uniform(0.0, 2.0 * np.pi, 16))
    rad = rng.uniform(0.8, 1.2, 16)             # star-shaped about its centre and counter-clockwise; not convex
    gon = np.stack([3.0 + rad * np.cos(ang), -2.0 + rad * np.sin(ang)], 1)
    arc = np.sort(rng.uniform(0.0, 0.5 * np.pi, 15))     # a corner and 15 points of a quarter ellipse: convex, and
    convex = np.concatenate([[[0.5, 0.25]],               # every s', t' >= 0, so that no sum cancels
                             np.stack([0.5 + 2.0 * np.cos(arc), 0.25 + 1.0 * np.sin(arc)], 1)])
    tri = np.array([[0.3, -0.2], [1.7, 0.1], [0.9, 1.4]])
    rep = np.array([[0.0, 0.0], [2.0, 0.0], [2.0, 0.0], [2.5, 1.0], [1.0, 2.0], [1.0, 2.0], [-0.5, 0.7]])
    rep0 = np.array([[0.1, 0.2], [0.1, 0.2], [1.5, 0.0], [2.0, 1.5], [0.4, 1.1]])     # vertex 0 itself repeated
    return dict(triangle=tri, star16=gon, convex16=convex, repeated=rep, repeated0=rep0)


@pytest.mark.parametrize("name", list(_polygons()))
def test_third_order_sums_of_the_fan_match_exact_polygon_integrals(name):
    """a, s, t, ss, st, tt, sss, sst, stt, ttt about vertex 0 against exact Fractions of the same doubles, to 1e-14 of the
    exact value; every value compared is at least 1e-3 of area * extent^order, so the relative bar means something."""
    poly = _polygons()[name]
    got = HMG.moments3(poly[:, 0], poly[:, 1])
    xs = [Fraction(float(x)) - Fraction(float(poly[0, 0])) for x in poly[:, 0]]
    ys = [Fraction(float(y)) - Fraction(float(poly[0, 1])) for y in poly[:, 1]]
    orders = ((0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2), (3, 0), (2, 1), (1, 2), (0, 3))
    area = float(_exact_monomial(xs, ys, 0, 0))
    extent = max(max(abs(float(x)) for x in xs), max(abs(float(y)) for y in ys))
    assert area > 0.0
    worst = 0.0
    for value, (i, j) in zip(got, orders):
        want = float(_exact_monomial(xs, ys, i, j))
        assert abs(want) >= 1e-3 * area * extent ** (i + j)
        worst = max(worst, abs(value - want) / abs(want))
    print(f"{name}: worst relative error of the ten sums = {worst:.3g}")
    assert worst <= 1e-14


# ---- closed form, identities ------------------------------------------------------------------------------------------

def test_the_cvt_energy_has_the_classical_gradient():
    c, fwd = H.case("uniform400"), HMG.host_forward("uniform400")
    grad = _host_grad(c, fwd, HMG.trace_upstream(fwd), None)
    assert HMG.check_closed_form(c, fwd, grad) >= 100


@pytest.mark.parametrize("name", HMG.IDENTITY_CASES)
def test_translation_and_scaling_identities(name):
    c, fwd = H.case(name), HMG.host_forward(name)
    assert fwd["bounded"].sum() >= (64 if name == "grid" else 300)
    gq, gc = HMG.unit_upstreams(fwd)
    HMG.check_identities(c["points"], fwd, gq, gc, _host_grad(c, fwd, gq, gc))
    for one in ((gq, None), (None, gc)):         # either upstream alone, the other absent
        HMG.check_identities(c["points"], fwd, *one, _host_grad(c, fwd, *one))


# ---- edge cases -------------------------------------------------------------------------------------------------------

def test_tiny_inputs_give_finite_numbers():
    tiny = H.tiny_inputs()
    for name in ("n1", "n2", "n4"):          # every cell is open: zeros, whatever arrives
        pts, off, adj = tiny[name]
        geo = H.cell_geometry(pts, adj, off)
        assert not geo["bounded"].any()
        n = len(pts)
        got = HMG.cell_moments_grad(pts, adj, off, geo, np.full((n, 6), np.inf), np.full((n, 6), np.nan))
        assert got["bad"] == 0 and got["grad"].shape == (n, 3) and (got["grad"] == 0.0).all()
    pts, off, adj = tiny["empty_row"]
    geo = H.cell_geometry(pts, adj, off)
    a = H.EMPTY_ROW_SITE
    assert not geo["bounded"][a] and geo["bounded"].sum() > 5
    gq, gc = HMG.unit_upstreams(geo)
    got = HMG.cell_moments_grad(pts, adj, off, geo, gq, gc)
    assert got["bad"] == 0 and np.isfinite(got["grad"]).all() and (got["grad"][a] == 0.0).all()
    assert np.abs(got["grad"]).max() > 0.0


def test_non_finite_upstreams_on_unbounded_cells_do_not_leak():
    c, geo = _rounded("uniform400")
    b = geo["bounded"]
    assert (~b).sum() > 20
    gq, gc = HMG.unit_upstreams(geo)                 # NaN on the unbounded cells
    clean = _host_grad(c, geo, np.where(b[:, None], gq, 0.0), np.where(b[:, None], gc, 0.0))
    for bad in (np.nan, np.inf, -np.inf):
        got = _host_grad(c, geo, np.where(b[:, None], gq, bad), np.where(b[:, None], gc, bad))
        assert np.array_equal(got, clean)
    assert np.isfinite(clean).all() and np.abs(clean[~b]).max() > 0.0     # open rows still carry their neighbours' terms


def test_a_257_gon_at_capacity_256_marks_the_axis_cells_and_leaves_the_rest():
    from radfoam_amd import foam

    pts = H._CLOUDS["ring257"]()
    off, adj = foam.delaunay_csr(pts)
    geo = H.cell_geometry(pts, adj, off, cap=512)          # a forward with room for the 257-gon: both axis cells bounded
    assert geo["bad"] == 0 and geo["bounded"][:2].all()
    gq, gc = HMG.unit_upstreams(geo)
    roomy = HMG.cell_moments_grad(pts, adj, off, geo, gq, gc, cap=512)
    got = HMG.cell_moments_grad(pts, adj, off, geo, gq, gc, cap=256)
    assert roomy["bad"] == 0 and np.isfinite(roomy["grad"]).all()
    assert got["bad"] == 2 and (got["status"][:2] == 1).all() and (got["status"][2:] == 0).all()
    assert np.isnan(got["grad"][:2]).all() and np.array_equal(got["grad"][2:], roomy["grad"][2:])


def test_malformed_rows_are_reported():
    c, geo = _rounded("ring16")
    adj = c["adjacency"].copy()
    off = c["offsets"].astype(np.int64)
    adj[off[3]] = 3                       # the site itself
    adj[off[7] + 1] = len(c["points"])    # past the end
    gq, gc = HMG.unit_upstreams(geo)
    got = HMG.cell_moments_grad(c["points"], adj, c["offsets"], geo, gq, gc)
    assert got["status"][3] == 2 and got["status"][7] == 2 and got["bad"] == 2
    assert np.isnan(got["grad"][[3, 7]]).all() and np.isfinite(np.delete(got["grad"], [3, 7], axis=0)).all()
