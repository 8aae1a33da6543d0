"""Second moments of the Voronoi cells, the part that runs without a GPU: radfoam_amd/csrc/rf_clip_moments.hpp compiled
for the host (tests/host_harness/clip_moments_host) against the exact rational reference (tests/cell_moments_ref.py), the
closed form on the unjittered grid, the scalings, the capacities, the degenerate inputs, and the Gaussians of
examples/foam_to_gaussians.py.  tests/test_gpu_cell_moments.py holds the device to the same bar.

The bar (clip_moments_host.check_against_exact): |delta| <= 1e-9 tr Q_exact[a] on each of the twelve numbers of cell a.
1e-9 is the bar of rf_clip.hpp against its exact reference; the unit is the exact site moment's trace, positive and of
the order length^5 (the cell's own s^5 is not used: on `clustered` tr Q / s^5 reaches 453).

Measured on the host, worst |d site| / tr Q and |d central| / tr Q:
  ring16 2.8e-15 2.8e-15, ring17 6.7e-15 4.1e-15, ring256 (axis cells) 9.8e-15 2.5e-15, hub64 9.7e-15 2.6e-15,
  hub65 6.1e-15 2.7e-15, hub200 2.3e-14 3.1e-15, redo_spread 1.4e-14 1.4e-14, uniform400 1.3e-14 5.7e-15,
  offset 7.6e-15 8.5e-13 (m = c - p is the difference of numbers near 2000), grid 1.0e-15 1.0e-15,
  clustered 1.1e-10 6.7e-11 (R = 4 |diagonal| is about 1e6 of its smallest cells, as for the volumes)."""
import os
from fractions import Fraction

import numpy as np
import pytest

from tests.host_harness import clip_host as H
from tests.host_harness import clip_moments_host as HM

_HOST = {}


def _host(name):
    """(case, host forward, host moments) of a case of clip_host.case, once"""
    if name not in _HOST:
        c, geo = H.case(name), HM.host_forward(name)
        _HOST[name] = (c, geo, HM.cell_moments(c["points"], c["adjacency"], c["offsets"], geo))
    return _HOST[name]


def test_sources_are_built_but_not_part_of_the_source_hash():
    from radfoam_amd import _lib, build

    names = lambda paths: {os.path.basename(p) for p in paths}
    assert "rf_cell_moments.hip" in names(build.EXTRA_SOURCES)
    assert {"rf_clip_moments.hpp", "radfoam_hip_moments.h"} <= names(build.EXTRA_HEADERS)
    assert not names(build.SOURCES + build.HEADERS) & names(build.EXTRA_SOURCES + build.EXTRA_HEADERS)
    lib = _lib.load()
    for name in ("rf_cell_moments", "rf_cell_moments_workspace_bytes"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.rf_cell_moments_workspace_bytes(1000) >= 1000
    none = [None] * 6
    assert lib.rf_cell_moments(None, 0, None, None, 0, None, *none, None, 0, None) == 0      # nothing to do
    assert lib.rf_cell_moments(None, 5, None, None, 0, None, *none, None, 0, None) == -1
    assert "null pointer" in _lib.last_error()
    dummy = np.zeros(64).ctypes.data
    assert lib.rf_cell_moments(dummy, 5, dummy, dummy, 4, dummy, *([dummy] * 6), dummy, 2, None) == -2
    assert "workspace" in _lib.last_error()


def test_public_names_and_input_checks_without_a_device():
    import torch

    import radfoam
    import radfoam_amd

    for name in ("cell_moments", "CellMoments"):
        assert name in radfoam.__all__ and name in radfoam_amd.__all__
    assert radfoam.CellMoments._fields == ("site_moment", "central_moment", "geometry")
    pts = torch.zeros(10, 3)
    adj, off = torch.zeros(5, dtype=torch.uint32), torch.zeros(11, dtype=torch.uint32)
    with pytest.raises(RuntimeError, match="points must be a float32 CUDA tensor"):
        radfoam.cell_moments(pts, adj, off)
    with pytest.raises(RuntimeError, match="points must be a float32 CUDA tensor"):
        radfoam.cell_moments(pts.double(), adj, off, geometry=None)
    geo = radfoam.CellGeometry(torch.zeros(10, dtype=torch.float64), torch.zeros(10, 3, dtype=torch.float64),
                               torch.zeros(10, dtype=torch.bool), torch.zeros(5, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="points must be a float32 CUDA tensor"):
        radfoam.cell_moments(pts, adj, off, geo)


def test_the_exact_reference_is_the_closed_form_on_the_grid_and_the_host_core_matches_it():
    """A cube of side h about its centre: int y_i^2 dy = h^5 / 12, the mixed moments vanish, and the centroid is the
    site, so site == central.  The rows of the interior sites also list diagonal neighbours whose faces have zero area
    (the cospherical grid): they must add exactly nothing."""
    c, geo, got = _host("grid")
    ref = HM.exact("grid")
    inner = H.grid_interior()
    assert inner.sum() == 64 and np.array_equal(ref["done"], inner)
    want = (Fraction(H.GRID_H) ** 5 / 12,) * 3 + (Fraction(0),) * 3
    for a in np.nonzero(inner)[0]:
        assert ref["site"][a] == want and ref["central"][a] == want
    rows = c["rows"]
    degree = np.bincount(rows, minlength=len(inner))
    assert (degree[inner] > 6).all()                    # zero-area faces are present in every interior row
    assert got["bad"] == 0 and geo["bounded"][inner].all()
    HM.check_against_exact("grid", geo["bounded"], got["site"], got["central"])
    h5 = H.GRID_H ** 5 / 12.0
    assert np.abs(got["site"][inner][:, :3] - h5).max() <= 1e-9 * 3 * h5
    assert np.abs(got["site"][inner][:, 3:]).max() <= 1e-9 * 3 * h5


@pytest.mark.parametrize("name", [n for n in HM.EXACT_CASES if n != "grid"])
def test_host_core_against_the_exact_reference(name):
    c, geo, got = _host(name)
    assert got["bad"] == 0 and (got["status"] == 0).all()
    HM.check_against_exact(name, geo["bounded"], got["site"], got["central"])
    seam = {"ring16": [0, 1], "ring17": [0, 1], "ring256": [0, 1], "hub64": [0], "hub65": [0], "hub200": [0],
            "redo_spread": list(np.array(H.REDO_SPREAD_PAIRS).reshape(-1))}.get(name)
    if seam is not None:                                 # the cells the case is about are among the compared
        HM.check_against_exact(name, geo["bounded"], got["site"], got["central"], cells=seam)
    # what the moments are for: the central moment is positive definite on a bounded cell, and the parallel-axis identity
    b = geo["bounded"]
    m = geo["centroid"][b] - c["points"][b].astype(np.float64)
    tr_site, tr_central = got["site"][b][:, :3].sum(1), got["central"][b][:, :3].sum(1)
    assert np.abs(tr_site - tr_central - geo["volume"][b] * (m * m).sum(1)).max() <= 1e-12 * tr_site.max()
    sym = np.empty((b.sum(), 3, 3))
    for k, (i, j) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        sym[:, i, j] = sym[:, j, i] = got["central"][b][:, k]
    assert (np.linalg.eigvalsh(sym)[:, 0] >= -1e-9 * tr_site).all()


@pytest.mark.parametrize("name,power", [("scaled_small", -10), ("scaled_large", 10)])
def test_a_power_of_two_scales_the_moments_bit_for_bit(name, power):
    """length^5: a power of two commutes with every operation of the headers"""
    c, geo, got = _host(name)
    _, base_geo, base = _host("uniform400")
    assert got["bad"] == 0 and np.array_equal(geo["bounded"], base_geo["bounded"]) and base_geo["bounded"].sum() > 300
    f = 2.0 ** (5 * power)
    assert np.array_equal(got["site"], base["site"] * f, equal_nan=True)
    assert np.array_equal(got["central"], base["central"] * f, equal_nan=True)


def test_a_257_gon_at_capacity_256_marks_the_axis_cells_and_leaves_the_rest():
    from radfoam_amd import foam

    pts = H._CLOUDS["ring257"]()
    off, adj = foam.delaunay_csr(pts)
    geo = H.cell_geometry(pts, adj, off, cap=512)          # a forward with room for the 257-gon: both axis cells bounded
    assert geo["bad"] == 0 and geo["bounded"][:2].all()
    roomy = HM.cell_moments(pts, adj, off, geo, cap=512)
    got = HM.cell_moments(pts, adj, off, geo, cap=256)
    assert roomy["bad"] == 0 and np.isfinite(roomy["site"][:2]).all()
    assert got["bad"] == 2 and (got["status"][:2] == 1).all() and (got["status"][2:] == 0).all()
    assert np.isnan(got["site"][:2]).all() and np.isnan(got["central"][:2]).all()
    assert np.array_equal(got["site"][2:], roomy["site"][2:], equal_nan=True)
    assert np.array_equal(got["central"][2:], roomy["central"][2:], equal_nan=True)
    assert np.isfinite(got["site"][2:]).any()


def test_a_malformed_row_is_status_2_bounded_or_not():
    c, geo, _ = _host("uniform400")
    adj = c["adjacency"].copy()
    inner, outer = int(np.nonzero(geo["bounded"])[0][0]), int(np.nonzero(~geo["bounded"])[0][0])
    for a in (inner, outer):
        adj[int(c["offsets"][a])] = a                       # the site itself in its own row
    got = HM.cell_moments(c["points"], adj, c["offsets"], geo)
    assert got["bad"] == 2 and got["status"][inner] == 2 and got["status"][outer] == 2
    assert np.isnan(got["site"][[inner, outer]]).all() and np.isnan(got["central"][[inner, outer]]).all()


def test_tiny_inputs():
    tiny = H.tiny_inputs()
    for name in ("n1", "n2", "n4"):                          # every cell is open
        pts, off, adj = tiny[name]
        geo = H.cell_geometry(pts, adj, off)
        got = HM.cell_moments(pts, adj, off, geo)
        assert got["bad"] == 0 and got["site"].shape == (len(pts), 6)
        assert np.isnan(got["site"]).all() and np.isnan(got["central"]).all()
    a = H.EMPTY_ROW_SITE
    out = {}
    for name in ("empty_row_full", "empty_row"):
        pts, off, adj = tiny[name]
        geo = H.cell_geometry(pts, adj, off)
        out[name] = (geo, HM.cell_moments(pts, adj, off, geo))
        assert out[name][1]["bad"] == 0
    (full_geo, full), (geo, got) = out["empty_row_full"], out["empty_row"]
    assert full_geo["bounded"][a] and np.isfinite(full["site"][a]).all() and not geo["bounded"][a]
    assert np.isnan(got["site"][a]).all() and np.isnan(got["central"][a]).all()
    # a cell is a gather over its own row: every other cell, the neighbours that still list the site included, carries
    # the bits of the full CSR
    rest = np.arange(len(geo["bounded"])) != a
    assert np.array_equal(got["site"][rest], full["site"][rest], equal_nan=True)
    assert np.array_equal(got["central"][rest], full["central"][rest], equal_nan=True)
    assert np.isfinite(got["site"][rest]).any()


def test_gaussians_from_the_moments_of_uniform400():
    import torch

    import radfoam
    from examples.foam_to_gaussians import gaussians_from_moments

    c, geo, got = _host("uniform400")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    moments = radfoam.CellMoments(t(got["site"]), t(got["central"]),
                                  radfoam.CellGeometry(t(geo["volume"]), t(geo["centroid"]), t(geo["bounded"]),
                                                       t(geo["face_area"])))
    g = gaussians_from_moments(moments)
    b = geo["bounded"]
    m = int(b.sum())
    assert np.array_equal(g["cell"].numpy(), np.nonzero(b)[0])
    assert np.array_equal(g["mean"].numpy(), geo["centroid"][b])
    scale, q = g["scale"].numpy(), g["rotation"].numpy()
    assert scale.shape == (m, 3) and q.shape == (m, 4)
    assert np.isfinite(scale).all() and (scale > 0.0).all()
    assert np.abs(np.linalg.norm(q, axis=1) - 1.0).max() <= 1e-12
    w, x, y, z = q.T
    rot = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                    np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                    np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)
    assert np.abs(np.linalg.det(rot) - 1.0).max() <= 1e-12
    want = np.empty((m, 3, 3))
    cov = got["central"][b] / geo["volume"][b][:, None]
    for k, (i, j) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        want[:, i, j] = want[:, j, i] = cov[:, k]
    back = np.einsum("mij,mj,mkj->mik", rot, scale ** 2, rot)
    worst = (np.abs(back - want).reshape(m, -1).max(1) / np.trace(want, axis1=1, axis2=2)).max()
    print(f"gaussians: {m} cells, worst |R diag(scale^2) R^T - central / V| / tr = {worst:.3g}")
    assert worst <= 1e-12
