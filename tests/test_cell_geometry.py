"""Voronoi cell geometry, the part that runs without a GPU: how the new kernel file is built, the input checks of the
Python layer, and the numerics of the clipping core (radfoam_amd/csrc/rf_clip.hpp, compiled for the host by
tests/host_harness/clip_host) against Qhull -- the same comparison tests/test_gpu_cell_geometry.py makes on the device."""
import os

import numpy as np
import pytest
import torch

from tests.host_harness import clip_host as H


def test_kernel_file_is_built_but_not_part_of_the_source_hash():
    from radfoam_amd import _lib, build

    names = lambda paths: {os.path.basename(p) for p in paths}
    assert "rf_cell_geometry.hip" in names(build.EXTRA_SOURCES)
    assert {"rf_clip.hpp", "radfoam_hip_geometry.h"} <= names(build.EXTRA_HEADERS)
    hashed = names(build.SOURCES + build.HEADERS)
    assert not hashed & names(build.EXTRA_SOURCES + build.EXTRA_HEADERS)
    for path in build.EXTRA_SOURCES + build.EXTRA_HEADERS:
        assert os.path.exists(path)
    # compiled and linked: the library exports what the file defines
    lib = _lib.load()
    for name in ("rf_cell_geometry", "rf_cell_geometry_workspace_bytes", "rf_cell_surface_count",
                 "rf_cell_surface_emit"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    # watched by needs_build(): a newer extra source makes the library stale
    newest = max(os.path.getmtime(p) for p in build.SOURCES + build.HEADERS + build.EXTRA_SOURCES + build.EXTRA_HEADERS)
    assert build.needs_build() == (newest > os.path.getmtime(build.OUTPUT))


def test_entry_points_validate_without_a_device():
    from radfoam_amd import _lib

    lib = _lib.load()
    assert lib.rf_cell_geometry_workspace_bytes(1000) >= 1000
    none = [None] * 6
    assert lib.rf_cell_geometry(None, 0, None, None, 0, None, *none, None, 0, None) == 0          # nothing to do
    assert lib.rf_cell_geometry(None, 5, None, None, 0, None, *none, None, 0, None) == -1
    assert "null pointer" in _lib.last_error()
    dummy = (torch.zeros(64, dtype=torch.float64)).numpy().ctypes.data
    assert lib.rf_cell_geometry(dummy, 5, dummy, dummy, 4, dummy, *([dummy] * 6), dummy, 2, None) == -2
    assert "workspace" in _lib.last_error()
    assert lib.rf_cell_surface_count(5, None, None, 0, None, None, None, None) == 0
    assert lib.rf_cell_surface_count(5, None, None, 3, None, None, None, None) == -1
    assert lib.rf_cell_surface_emit(None, 5, None, None, 3, None, None, None, None, 0, None, None, None) == 0
    assert lib.rf_cell_surface_emit(None, 5, None, None, 3, None, None, None, None, 2, None, None, None) == -1


def test_cpu_tensors_are_refused_like_farthest_neighbor():
    import radfoam
    from radfoam_amd import scene_ops

    pts = torch.zeros(10, 3)
    adj, off = torch.zeros(5, dtype=torch.uint32), torch.zeros(11, dtype=torch.uint32)
    with pytest.raises(RuntimeError) as want:
        scene_ops.farthest_neighbor(pts, adj, off)
    with pytest.raises(RuntimeError) as got:
        radfoam.cell_geometry(pts, adj, off)
    assert str(got.value) == str(want.value) == "points must be a float32 CUDA tensor"
    with pytest.raises(RuntimeError, match="points must be a float32 CUDA tensor"):
        radfoam.cell_surface(pts, adj, off, torch.zeros(10, dtype=torch.bool))
    assert radfoam.CellGeometry._fields == ("volume", "centroid", "bounded", "face_area")


@pytest.mark.parametrize("name", ["uniform", "ring"])
def test_clipping_core_on_the_host_matches_qhull(name):
    c = H.case(name)
    got = H.cell_geometry(c["points"], c["adjacency"], c["offsets"])
    assert got["bad"] == 0
    if name == "uniform":
        assert c["ref"]["compared"].sum() >= 0.8 * c["points"].shape[0]
    else:
        assert c["ref"]["ridge_vertices"][(0, 1)] == 48 and c["ref"]["compared"][:2].all()
        slot = int(c["offsets"][0]) + int(np.searchsorted(c["adjacency"][c["offsets"][0]:c["offsets"][1]], 1))
        assert got["face_vertices"][slot] == 48
    H.check_cells(c, got["volume"], got["centroid"], got["bounded"])
    H.check_faces(c, got["volume"], got["bounded"], got["face_area"])
    # the polygons have Qhull's vertex counts wherever both cells are bounded
    both = got["bounded"][c["rows"]] & got["bounded"][c["adjacency"]]
    want = np.array([c["ref"]["ridge_vertices"].get((int(a), int(b)), 0)
                     for a, b in zip(c["rows"][both], c["adjacency"][both])])
    assert (got["face_vertices"][both] == want).all()


def test_a_polygon_capacity_below_the_face_is_reported_never_a_wrong_number():
    c = H.case("ring")
    for cap in (16, 47):
        got = H.cell_geometry(c["points"], c["adjacency"], c["offsets"], cap=cap)
        assert (got["status"][:2] == 1).all() and np.isnan(got["volume"][:2]).all() and not got["bounded"][:2].any()
        ok = got["status"] == 0
        full = H.cell_geometry(c["points"], c["adjacency"], c["offsets"])
        assert np.array_equal(got["volume"][ok], full["volume"][ok])


def test_malformed_rows_are_reported():
    c = H.case("ring")
    adj = c["adjacency"].copy()
    off = c["offsets"].astype(np.int64)
    adj[off[3]] = 3                       # the site itself
    adj[off[7] + 1] = len(c["points"])    # past the end
    got = H.cell_geometry(c["points"], adj, c["offsets"])
    assert got["status"][3] == 2 and got["status"][7] == 2 and got["bad"] == 2


def test_face_polygons_are_wound_from_a_to_b():
    c = H.case("uniform")
    pts = c["points"].astype(np.float64)
    inside = np.linalg.norm(pts, axis=1) < 0.5
    slots = np.nonzero(inside[c["rows"]] & ~inside[c["adjacency"]])[0][:200]
    for e in slots:
        a, b = int(c["rows"][e]), int(c["adjacency"][e])
        poly = H.face_polygon(c["points"], c["adjacency"], c["offsets"], a, int(e))
        normal = np.cross(poly[1:-1] - poly[0], poly[2:] - poly[0])
        assert (normal @ (pts[b] - pts[a]) > 0).all()


# ---- the exact reference (tests/cell_geometry_ref.py) and the clouds that stand on the kernel's seams --------------------
#
# Worst ratios of the host build against the exact reference, in units of each cell's own size (bar 1e-9):
#   ring16/17 |dV| 1e-14, ring256 |dV| 9e-14 |dc| 2e-13 |dA| 2e-13, hub64/65/200 |dV| 2e-14 |dA| 1e-13,
#   uniform400 / scaled_* |dV| 1e-14, offset |dc| 2e-13, redo_spread |dV| 1e-14 |dA| 8e-14, grid |dV| 2e-15,
#   clustered |dV| 1.2e-10 |dc| 4.4e-11 |dA| 2.9e-10 symmetry 4.2e-10 closure 4.3e-10 (R = 4 |diagonal| is 1e6 times its
#   smallest cells; still under the bar, so no Qhull yardstick was needed).

from fractions import Fraction

from tests import cell_geometry_ref as X

EXACT_CASES = ["ring16", "ring17", "ring256", "hub64", "hub65", "hub200", "redo_spread", "clustered", "uniform400",
               "offset", "scaled_small", "scaled_large"]
_HOST = {}


def _host(name, cap=256):
    if (name, cap) not in _HOST:
        c = H.case(name)
        _HOST[(name, cap)] = H.cell_geometry(c["points"], c["adjacency"], c["offsets"], cap=cap)
    return _HOST[(name, cap)]


def test_exact_reference_returns_the_closed_form_on_a_grid():
    c = H.case("grid")
    ex, h = c["exact"], Fraction(1, 4)
    inner = H.grid_interior()
    assert inner.sum() == 64 and np.array_equal(~ex["open"], inner)
    pts = c["points"]
    for a in np.nonzero(inner)[0]:
        assert ex["volume"][a] == h ** 3
        assert ex["centroid"][a] == tuple(Fraction(float(x)) for x in pts[a])
        lo, hi = int(c["offsets"][a]), int(c["offsets"][a + 1])
        areas = c["slots"]["area"][lo:hi]
        axis = np.abs(pts[c["adjacency"][lo:hi]] - pts[a]).sum(1) == 0.25
        assert axis.sum() == 6 and (areas[axis] == 0.0625).all() and (areas[~axis] == 0.0).all()
    assert (c["slots"]["area"][inner[c["rows"]]] == 0.0).sum() > 0        # the triangulated adjacency lists diagonals


@pytest.mark.parametrize("k", [16, 17, 256, 257])
def test_ring_clouds_share_a_k_gon_that_never_needs_more_room(k):
    c = H.case(f"ring{k}")
    ex = c["exact"]
    assert not ex["open"][:k + 2].any() and ex["open"][k + 2:].all()           # axis and ring cells bounded: k + 2
    assert ex["faces"][(0, 1)][1] == k
    assert (ex["extent"][:k + 2] < 0.5 * c["R"]).all()
    if k == 16:     # the axis cells stay on the lane path: no face of theirs has more than kLaneCap vertices
        for a in (0, 1):
            assert c["slots"]["vertices"][int(c["offsets"][a]):int(c["offsets"][a + 1])].max() == 16
    assert (_host(f"ring{k}", cap=k)["status"][:2] == 0).all()
    assert (_host(f"ring{k}", cap=k - 1)["status"][:2] == 1).all()
    got = _host(f"ring{k}", cap=k)
    assert got["face_vertices"][H.slot_of(c, 0, 1)] == k == got["face_vertices"][H.slot_of(c, 1, 0)]


@pytest.mark.parametrize("k", [64, 65, 200])
def test_hub_clouds_give_the_centre_a_row_of_exactly_k(k):
    c = H.case(f"hub{k}")
    ex = c["exact"]
    assert int(c["offsets"][1]) - int(c["offsets"][0]) == k
    assert np.array_equal(c["adjacency"][:k], np.arange(1, k + 1))
    assert not ex["open"][:k + 1].any() and (ex["extent"][:k + 1] < 0.5 * c["R"]).all()
    assert (c["slots"]["vertices"][:k] >= 3).all()


def test_redo_spread_puts_17_gons_in_three_blocks_of_the_redo_kernel():
    c = H.case("redo_spread")
    blocks = [a // 64 for a, _ in H.REDO_SPREAD_PAIRS]
    assert blocks == [b // 64 for _, b in H.REDO_SPREAD_PAIRS] == [0, 0, 1, 3]
    for a, b in H.REDO_SPREAD_PAIRS:
        assert c["exact"]["faces"][(a, b)][1] == 17 and not c["exact"]["open"][[a, b]].any()
    assert not c["exact"]["open"][:74].any()


def test_the_other_clouds_are_what_they_claim():
    c = H.case("clustered")
    size = np.cbrt(c["exact"]["volume_f"][~c["exact"]["open"]])
    assert len(c["points"]) == 600 and (~c["exact"]["open"]).sum() >= 500 and size.max() / size.min() > 1e4
    base = H.case("uniform400")
    assert (~base["exact"]["open"]).sum() >= 300
    for name, f in (("scaled_small", 2.0 ** -10), ("scaled_large", 2.0 ** 10)):
        s = H.case(name)
        assert np.array_equal(s["points"].astype(np.float64), base["points"].astype(np.float64) * f)
        assert np.array_equal(s["adjacency"], base["adjacency"]) and np.array_equal(s["offsets"], base["offsets"])
        # the reference says exactly how the outputs scale
        assert all(v == w * Fraction(f) ** 3 for v, w in zip(s["exact"]["volume"], base["exact"]["volume"])
                   if w is not None)
    assert (~H.case("offset")["exact"]["open"]).sum() >= 300
    assert np.abs(H.case("offset")["points"]).min(0).tolist() > [900.0, 1900.0, 400.0]


@pytest.mark.parametrize("name", EXACT_CASES)
def test_clipping_core_on_the_host_matches_the_exact_reference(name):
    share = None if name == "clustered" else 0.05
    H.check_against_exact(H.case(name), _host(name), share=share)


def test_257_vertices_are_reported_and_every_other_cell_is_untouched():
    c = H.case("ring257")
    got, full = _host("ring257"), _host("ring257", cap=300)
    assert (got["status"][:2] == 1).all() and (got["status"][2:] == 0).all() and got["bad"] == 2
    assert np.isnan(got["volume"][:2]).all() and not got["bounded"][:2].any()
    ok = got["status"] == 0
    for key in ("volume", "centroid", "bounded"):
        assert np.array_equal(got[key][ok], full[key][ok], equal_nan=True)
    of_ok = ok[c["rows"]]
    assert np.array_equal(got["face_area"][of_ok], full["face_area"][of_ok])
    H.check_against_exact(c, full)                       # and with room for it the 257-gon is right


@pytest.mark.parametrize("k", [64, 65, 200])
def test_hub_centre_on_the_host(k):
    c, got = H.case(f"hub{k}"), _host(f"hub{k}")
    assert np.isfinite(got["face_area"][:k]).all() and (got["face_area"][:k] > 0).all()
    assert np.array_equal(got["face_vertices"][:k].astype(np.int64), c["slots"]["vertices"][:k])
    H.check_against_exact(c, got, cells=np.arange(k + 1))


def test_power_of_two_scaling_commutes_bit_for_bit_on_the_host():
    base = _host("uniform400")
    for name, f in (("scaled_small", 2.0 ** -10), ("scaled_large", 2.0 ** 10)):
        got = _host(name)
        assert np.array_equal(got["volume"], base["volume"] * f ** 3)
        assert np.array_equal(got["centroid"], base["centroid"] * f, equal_nan=True)
        assert np.array_equal(got["face_area"], base["face_area"] * f ** 2)


def test_grid_of_cospherical_sites_on_the_host():
    c, got = H.case("grid"), _host("grid")
    assert got["bad"] == 0
    H.check_grid(c, got)
    H.check_against_exact(c, got, vertices=False)


def test_tiny_inputs_on_the_host():
    tiny = H.tiny_inputs()
    got = H.cell_geometry(*[tiny["n4"][i] for i in (0, 2, 1)])
    assert got["bad"] == 0 and not got["bounded"].any() and np.isposinf(got["volume"]).all()
    assert np.isnan(got["centroid"]).all() and np.isposinf(got["face_area"]).all()
    for name in ("n1", "n2"):
        got = H.cell_geometry(*[tiny[name][i] for i in (0, 2, 1)])
        assert got["bad"] == 0 and not got["bounded"].any() and np.isposinf(got["volume"]).all()
    a = H.EMPTY_ROW_SITE
    full = H.cell_geometry(*[tiny["empty_row_full"][i] for i in (0, 2, 1)])
    got = H.cell_geometry(*[tiny["empty_row"][i] for i in (0, 2, 1)])
    assert full["bounded"][a] and full["bounded"].sum() > 5
    assert got["bad"] == 0 and not got["bounded"][a] and np.isposinf(got["volume"][a]) and np.isnan(got["centroid"][a]).all()
    rest = np.arange(len(full["volume"])) != a
    for key in ("volume", "centroid", "bounded"):
        assert np.array_equal(got[key][rest], full[key][rest], equal_nan=True)


def test_surfaces_on_the_host():
    c = H.case("hub200")
    inside = np.zeros(len(c["points"]), dtype=bool)
    inside[0] = True
    tri, edge = H.host_surface(c, inside)
    assert len(edge) == (c["slots"]["vertices"][:200] - 2).sum()
    H.check_surface(c, inside, tri, edge, c["exact"]["volume_f"][0], np.cbrt(c["exact"]["volume_f"][0]))
    c = H.case("grid")
    block = np.zeros((6, 6, 6), dtype=bool)
    block[2:4, 2:4, 2:4] = True
    tri, edge = H.host_surface(c, block.reshape(-1))
    H.check_surface(c, block.reshape(-1), tri, edge, 8 * H.GRID_H ** 3, H.GRID_H, area=24 * H.GRID_H ** 2,
                    counts=False)      # zero-area faces of cospherical sites have whatever count they have
    c = H.case("ring17")
    inside = np.zeros(len(c["points"]), dtype=bool)
    inside[1] = True
    tri, edge = H.host_surface(c, inside)
    assert (edge == H.slot_of(c, 1, 0)).sum() == 15
    H.check_surface(c, inside, tri, edge, c["exact"]["volume_f"][1], np.cbrt(c["exact"]["volume_f"][1]))
