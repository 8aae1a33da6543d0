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
