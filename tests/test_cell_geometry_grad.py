"""Point gradients of the cell geometry, the part that runs without a GPU: radfoam_amd/csrc/rf_clip_grad.hpp compiled for
the host (tests/host_harness/clip_grad_host) against difference quotients of the exact rational geometry
(tests/cell_geometry_grad_ref.py), the translation and scaling identities, one cell's volume against the exact faces,
and the degenerate inputs.  tests/test_gpu_cell_geometry_grad.py holds the device to the same bars.

L sums over the cells the host forward calls bounded: a cell the exact reference calls bounded may come out open where it
reaches past R / 2 (tests/test_cell_geometry.py, "either way"), its phi is then zero by definition, and the upstreams of
the reference are zero there.

Measured on the host (spread / max |R| of the reference, then the worst |<grad, delta> - R| / spread over the probes):
  uniform400 1.7e-7 2.9e-6, hub64 7.7e-10 2.7e-3, hub65 6.9e-10 3.7e-3, ring16 4.1e-10 1.4e-2, ring17 6.8e-9 8.6e-3,
  redo_spread 5.6e-8 3.4e-3 (the worst ratios are on the single-coordinate probes, whose spread is 1e-13 .. 1e-11)."""
import os

import numpy as np
import pytest

from tests import cell_geometry_grad_ref as G
from tests.host_harness import clip_grad_host as HG
from tests.host_harness import clip_host as H


def _rounded(name):
    """(case on the 2^-16 grid, host forward)"""
    c = G.case(name)
    return c, HG.host_forward(("rounded", name), c)


def _host_grad(c, geo, gv, gc, cap=256):
    got = HG.cell_geometry_grad(c["points"], c["adjacency"], c["offsets"], geo, gv, gc, cap=cap)
    assert got["bad"] == 0
    return got["grad"]


def test_sources_are_built_but_not_part_of_the_source_hash():
    from radfoam_amd import _lib, build

    names = lambda paths: {os.path.basename(p) for p in paths}
    assert "rf_cell_geometry_grad.hip" in names(build.EXTRA_SOURCES)
    assert {"rf_clip_grad.hpp", "rf_cell_wave.hpp", "radfoam_hip_geometry_grad.h"} <= names(build.EXTRA_HEADERS)
    assert not names(build.SOURCES + build.HEADERS) & names(build.EXTRA_SOURCES + build.EXTRA_HEADERS)
    lib = _lib.load()
    for name in ("rf_cell_geometry_grad", "rf_cell_geometry_grad_workspace_bytes"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.rf_cell_geometry_grad_workspace_bytes(1000) >= 1000
    none = [None] * 7
    assert lib.rf_cell_geometry_grad(None, 0, None, None, 0, None, *none, None, 0, None) == 0      # nothing to do
    assert lib.rf_cell_geometry_grad(None, 5, None, None, 0, None, *none, None, 0, None) == -1
    assert "null pointer" in _lib.last_error()
    dummy = np.zeros(64).ctypes.data
    assert lib.rf_cell_geometry_grad(dummy, 5, dummy, dummy, 4, dummy, *([dummy] * 7), dummy, 2, None) == -2
    assert "workspace" in _lib.last_error()


def test_public_names_and_input_checks_without_a_device():
    import torch

    import radfoam

    assert callable(radfoam.cell_geometry_grad) and callable(radfoam.differentiable_cell_geometry)
    pts = torch.zeros(10, 3)
    adj, off = torch.zeros(5, dtype=torch.uint32), torch.zeros(11, dtype=torch.uint32)
    with pytest.raises(RuntimeError, match="points must be a float32 CUDA tensor"):
        radfoam.differentiable_cell_geometry(pts, adj, off)
    with pytest.raises(RuntimeError, match="points must be a float32 CUDA tensor"):
        radfoam.cell_geometry_grad(pts, adj, off, None, None, None)


def test_rounded_clouds_keep_what_makes_them_seams():
    """from the exact reference alone"""
    for k in (64, 65):
        c = G.case(f"hub{k}")
        assert len(G.faces_of(c, 0)) == k == int(c["offsets"][1]) and not c["exact"]["open"][:k + 1].any()
    for k in (16, 17):
        c = G.case(f"ring{k}")
        assert c["exact"]["faces"][(0, 1)][1] == k and not c["exact"]["open"][:2].any()
    c = G.case("redo_spread")
    for a, b in H.REDO_SPREAD_PAIRS:
        assert c["exact"]["faces"][(a, b)][1] == 17 and not c["exact"]["open"][[a, b]].any()
    assert (~G.case("uniform400")["exact"]["open"]).sum() == 352
    for name in G.FD_CASES:
        p = G.case(name)["points"].astype(np.float64) * 2.0 ** G.GRID_BITS
        assert np.array_equal(p, np.round(p))


@pytest.mark.parametrize("name", G.FD_CASES)
def test_gradient_matches_difference_quotients_of_the_exact_geometry(name):
    c, geo = _rounded(name)
    cells = geo["bounded"]
    assert not c["exact"]["open"][cells].any() and cells.sum() >= 0.9 * (~c["exact"]["open"]).sum()
    if name != "uniform400":       # the seam cells are in L
        assert cells[[s for s, _ in G.SEAM_PROBES[name]]].all()
    ref, rec = G.reference(name, cells), G.recorded(name)
    assert np.array_equal(rec["cells"], cells) and np.array_equal(rec["R"], ref["R"])          # the record the GPU
    assert np.array_equal(rec["spread"], ref["spread"]) and np.array_equal(rec["w"], ref["w"])   # tests read
    grad = _host_grad(c, geo, ref["w"], ref["u"])
    G.check_against_reference(name, ref, grad)
    # the same through a capacity that just fits, and a capacity below the face is reported, never a wrong number
    if name in ("ring16", "ring17"):
        k = int(name[4:])
        fits = HG.cell_geometry_grad(c["points"], c["adjacency"], c["offsets"], geo, ref["w"], ref["u"], cap=k)
        assert (fits["status"][:2] == 0).all() and np.array_equal(fits["grad"][:2], grad[:2])
        small = HG.cell_geometry_grad(c["points"], c["adjacency"], c["offsets"], geo, ref["w"], ref["u"], cap=k - 1)
        assert (small["status"][:2] == 1).all() and np.isnan(small["grad"][:2]).all()
        ok = small["status"] == 0
        assert np.array_equal(small["grad"][ok], grad[ok])


@pytest.mark.parametrize("name", ["uniform", "offset", "clustered", "grid"])
def test_translation_and_scaling_identities(name):
    c = H.case(name)
    geo = HG.host_forward(("plain", name), c)
    assert geo["bounded"].sum() >= (64 if name == "grid" else 300)
    gv, gc = HG.unit_upstreams(geo)
    grad = _host_grad(c, geo, gv, gc)
    HG.check_identities(c["points"], geo, gv, gc, grad)
    for one in ((gv, None), (None, gc)):         # either upstream alone, the other absent
        part = _host_grad(c, geo, *one)
        zero = (np.where(geo["bounded"], 0.0, np.nan), np.where(geo["bounded"][:, None], np.zeros((1, 3)), np.nan))
        HG.check_identities(c["points"], geo, one[0] if one[0] is not None else zero[0],
                            one[1] if one[1] is not None else zero[1], part)


def test_face_moments_of_a_polygon_match_its_triangles():
    """A, m and S of the fan against Gauss quadrature of the same polygon's triangles (degree 2: edge midpoints)"""
    c = H.case("uniform400")
    geo = HG.host_forward(("plain", "uniform400"), c)
    a = int(np.nonzero(geo["bounded"])[0][5])
    for e in range(int(c["offsets"][a]), int(c["offsets"][a + 1])):
        poly = H.face_polygon(c["points"], c["adjacency"], c["offsets"], a, e) - c["points"][a].astype(np.float64)
        A, m, S = HG.face_moments(c["points"], c["adjacency"], c["offsets"], a, e)
        wa, wm, wS = 0.0, np.zeros(3), np.zeros((3, 3))
        for k in range(1, len(poly) - 1):
            tri = poly[[0, k, k + 1]]
            area = 0.5 * np.linalg.norm(np.cross(tri[1] - tri[0], tri[2] - tri[0]))
            mids = 0.5 * (tri + np.roll(tri, 1, axis=0))
            wa, wm, wS = wa + area, wm + area * mids.mean(0), wS + area / 3.0 * mids.T @ mids
        s = np.cbrt(geo["volume"][a])
        assert abs(A - wa) <= 1e-12 * s ** 2 and np.abs(m - wm).max() <= 1e-12 * s ** 3
        assert np.abs(S - wS).max() <= 1e-12 * s ** 4


def test_one_cells_volume_moves_its_neighbours_by_the_exact_faces():
    """gC = 0 and gV = 1 on one cell a: grad p_b = A_ab (p_b - c_ab) / l on every neighbour b, the face taken from the
    exact reference; grad p_a closes the sum (translation); every other row is exactly zero."""
    c, geo = _rounded("uniform400")
    p = c["points"].astype(np.float64)
    for a in np.nonzero(geo["bounded"])[0][[3, 77]]:
        a = int(a)
        gv = np.zeros(len(p))
        gv[a] = 1.0
        grad = _host_grad(c, geo, gv, np.zeros((len(p), 3)))
        nbrs = c["adjacency"][int(c["offsets"][a]):int(c["offsets"][a + 1])].astype(np.int64)
        s = np.cbrt(c["exact"]["volume_f"][a])
        worst = 0.0
        for b in nbrs:
            area, centre = G.exact_face(c["points"], a, int(b))
            assert area == pytest.approx(c["exact"]["faces"][(min(a, b), max(a, b))][0], rel=1e-12, abs=1e-300)
            want = area * (p[b] - centre) / np.linalg.norm(p[b] - p[a])
            worst = max(worst, np.abs(grad[b] - want).max() / s ** 2)
        print(f"cell {a}: {len(nbrs)} neighbours, worst |grad p_b - A (p_b - c_ab) / l| = {worst:.3g} s^2")
        assert worst <= 1e-9
        assert np.abs(grad[a] + grad[nbrs].sum(0)).max() <= 1e-9 * s ** 2
        off_row = np.ones(len(p), dtype=bool)
        off_row[nbrs] = off_row[a] = False
        assert (grad[off_row] == 0.0).all()


def test_tiny_inputs_give_finite_numbers():
    tiny = H.tiny_inputs()
    for name in ("n1", "n2", "n4"):          # every cell is open: zeros, whatever arrives
        pts, off, adj = tiny[name]
        geo = H.cell_geometry(pts, adj, off)
        assert not geo["bounded"].any()
        n = len(pts)
        got = HG.cell_geometry_grad(pts, adj, off, geo, np.full(n, np.inf), np.full((n, 3), np.nan))
        assert got["bad"] == 0 and (got["grad"] == 0.0).all()
    pts, off, adj = tiny["empty_row"]
    geo = H.cell_geometry(pts, adj, off)
    a = H.EMPTY_ROW_SITE
    assert not geo["bounded"][a] and geo["bounded"].sum() > 5
    gv, gc = HG.unit_upstreams(geo)
    got = HG.cell_geometry_grad(pts, adj, off, geo, gv, gc)
    assert got["bad"] == 0 and np.isfinite(got["grad"]).all() and (got["grad"][a] == 0.0).all()
    # the rows that list the site still carry their own terms of it: they equal the full CSR's rows wherever neither the
    # row's cell nor a neighbour of it changed its boundedness
    pts, off_f, adj_f = tiny["empty_row_full"]
    full_geo = H.cell_geometry(pts, adj_f, off_f)
    assert np.isfinite(HG.cell_geometry_grad(pts, adj_f, off_f, full_geo, *HG.unit_upstreams(full_geo))["grad"]).all()


def test_non_finite_upstreams_on_unbounded_cells_do_not_leak():
    c, geo = _rounded("uniform400")
    b = geo["bounded"]
    assert (~b).sum() > 20
    gv, gc = HG.unit_upstreams(geo)                 # NaN on the unbounded cells
    clean = _host_grad(c, geo, np.where(b, gv, 0.0), np.where(b[:, None], gc, 0.0))
    for bad in (np.nan, np.inf, -np.inf):
        got = _host_grad(c, geo, np.where(b, gv, bad), np.where(b[:, None], gc, bad))
        assert np.array_equal(got, clean)
    assert np.isfinite(clean).all() and np.abs(clean[~b]).max() > 0.0     # open rows still carry their neighbours' terms


def test_malformed_rows_are_reported():
    c, geo = _rounded("ring16")
    adj = c["adjacency"].copy()
    off = c["offsets"].astype(np.int64)
    adj[off[3]] = 3                       # the site itself
    adj[off[7] + 1] = len(c["points"])    # past the end
    gv, gc = HG.unit_upstreams(geo)
    got = HG.cell_geometry_grad(c["points"], adj, c["offsets"], geo, gv, gc)
    assert got["status"][3] == 2 and got["status"][7] == 2 and got["bad"] == 2
    assert np.isnan(got["grad"][[3, 7]]).all() and np.isfinite(np.delete(got["grad"], [3, 7], axis=0)).all()
