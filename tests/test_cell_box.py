"""Voronoi cells clipped to a box (radfoam.cell_geometry_in_box), the part that runs without a GPU: how the new kernel
file is built, the box's validation, and the numerics of radfoam_amd/csrc/rf_clip_box.hpp, compiled for the host by
tests/host_harness/clip_box_host, against the exact rational reference of tests/cell_box_ref.py and the identities a
partition of the box obeys -- the checks tests/test_gpu_cell_box.py makes on the device, through the same functions."""
import os

import numpy as np
import pytest
import torch

from tests.host_harness import clip_box_host as B
from tests.host_harness import clip_host as H


def test_kernel_file_is_built_but_not_part_of_the_source_hash():
    from radfoam_amd import _lib, build

    names = lambda paths: {os.path.basename(p) for p in paths}
    assert "rf_cell_box.hip" in names(build.EXTRA_SOURCES)
    assert {"rf_clip_box.hpp", "radfoam_hip_box.h"} <= names(build.EXTRA_HEADERS)
    assert not names(build.SOURCES + build.HEADERS) & {"rf_cell_box.hip", "rf_clip_box.hpp", "radfoam_hip_box.h"}
    lib = _lib.load()
    for name in ("rf_cell_box", "rf_cell_box_workspace_bytes"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)


def test_entry_point_validates_without_a_device():
    from radfoam_amd import _lib

    lib = _lib.load()
    assert lib.rf_cell_box_workspace_bytes(1000) >= 1000
    unit, none = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0), [None] * 8
    assert lib.rf_cell_box(None, 0, None, None, 0, None, *unit, *none, None, 0, None) == 0          # nothing to do
    assert lib.rf_cell_box(None, 5, None, None, 0, None, *unit, *none, None, 0, None) == -1
    assert "null pointer" in _lib.last_error()
    dummy = (torch.zeros(64, dtype=torch.float64)).numpy().ctypes.data
    for box in ((0.0, 0.0, 0.0, 1.0, 0.0, 1.0), (0.0, 0.0, 0.0, 1.0, float("nan"), 1.0),
                (0.0, 0.0, -float("inf"), 1.0, 1.0, 1.0)):
        assert lib.rf_cell_box(dummy, 5, dummy, dummy, 4, dummy, *box, *([dummy] * 8), dummy, 4096, None) == -1
        assert "lo < hi" in _lib.last_error()
    assert lib.rf_cell_box(dummy, 5, dummy, dummy, 4, dummy, *unit, *([dummy] * 8), dummy, 2, None) == -2
    assert "workspace" in _lib.last_error()


def test_the_box_is_validated_before_anything_else():
    """lo >= hi, NaN, inf and a wrong length raise ValueError; nothing is launched (the tensors are not even looked at)"""
    import radfoam
    from radfoam_amd import geometry

    assert "cell_geometry_in_box" in radfoam.__all__ and "BoxedCellGeometry" in radfoam.__all__
    for bad in ((0, 0, 0, 1, 1), (0, 0, 0, 1, 1, 1, 1), (0, 0, 0, 1, 0, 1), (0, 0, 0, 1, -1, 1), (0, 0, 0, 1, float("nan"), 1),
                (0, 0, -float("inf"), 1, 1, 1), torch.zeros(2, 3), torch.zeros(5), "box", None, (-1e308, 0, 0, 1e308, 1, 1)):
        with pytest.raises(ValueError, match="box must"):
            radfoam.cell_geometry_in_box(None, None, None, bad)
    want = [-1.0, -2.0, -3.0, 1.0, 2.0, 3.0]
    for good in (want, tuple(want), torch.tensor(want), torch.tensor(want, dtype=torch.float64).reshape(2, 3),
                 np.array(want).reshape(2, 3), (want[:3], want[3:])):
        assert geometry._box_six(good) == want
    with pytest.raises(RuntimeError, match="points must be a float32 CUDA tensor"):
        radfoam.cell_geometry_in_box(torch.zeros(4, 3), torch.zeros(0, dtype=torch.int32),
                                     torch.zeros(5, dtype=torch.int32), want)


# ---- 1. the exact reference ------------------------------------------------------------------------------------------

def test_the_reference_works_on_cells_of_every_kind():
    """uniform400 in [-1,1]^3: at least 40 cells that touch a wall, among them cells touching two and three, and 10 that
    touch none; the tight box leaves 300 of the 400 sites outside and 10 empty cells are among the reference's; the disjoint box has
    3 non-empty cells"""
    ref = B.exact("uniform400")
    touched = (ref["wall_area"][ref["done"]] > 0).sum(1)
    assert (touched >= 1).sum() >= 40 and (touched == 2).sum() >= 1 and (touched >= 3).sum() >= 1
    assert (touched == 0).sum() >= 10
    c, ref = B.case("tight"), B.exact("tight")
    p, box = c["points"].astype(np.float64), c["box"]
    assert ((p < box[:3]) | (p > box[3:])).any(1).sum() == 300
    assert (ref["volume_f"][ref["done"]] == 0.0).sum() >= 10
    assert (B.host("disjoint")["nonempty"]).sum() == 3
    assert set(np.nonzero(B.host("disjoint")["nonempty"])[0]) <= set(np.nonzero(B.exact("disjoint")["done"])[0])


@pytest.mark.parametrize("name", ["uniform400", "tight", "wide", "disjoint", "offset", "scaled_small", "scaled_large"])
def test_cells_in_a_box_against_the_exact_reference(name):
    out = B.host(name)
    assert out["bad"] == 0
    B.check_against_exact(name, out)


@pytest.mark.parametrize("name,power", [("scaled_small", -10), ("scaled_large", 10)])
def test_a_power_of_two_scales_the_results_bit_for_bit(name, power):
    out, base = B.host(name), B.host("uniform400")
    f = 2.0 ** power
    assert np.array_equal(out["volume"], base["volume"] * f ** 3) and np.array_equal(out["centroid"], base["centroid"] * f)
    assert np.array_equal(out["face_area"], base["face_area"] * f ** 2)
    assert np.array_equal(out["wall_area"], base["wall_area"] * f ** 2)
    assert np.array_equal(out["face_vertices"], base["face_vertices"])


# ---- 2. identities on whole clouds -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["uniform400", "tight", "wide", "disjoint", "offset", "hub58", "hub59", "ring16", "ring17",
                                  "ring256", "redo_spread"])
def test_the_cells_partition_the_box(name):
    out = B.host(name)
    assert out["bad"] == 0
    B.check_identities(B.case(name), out)


# ---- 3. agreement with cell_geometry ---------------------------------------------------------------------------------

def test_cells_that_touch_no_wall_agree_with_cell_geometry():
    for name, share in (("wide", 0.25), ("uniform400", None), ("offset", None)):
        c = B.case(name)
        B.check_agreement(c, B.host(name), B.host_geometry(B.CASES[name][0]), share=share)


# ---- 4. seams ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [58, 59])
def test_a_list_of_64_planes_and_one_of_65(k):
    """hub58's site 0 has 58 neighbours and 6 walls, the last list the lane-per-face kernel takes; hub59's is the first the
    serial path takes.  The +x wall cuts the hub cell in a 14-gon / 15-gon."""
    name = f"hub{k}"
    c, ref, out = B.case(name), B.exact(name), B.host(name)
    degrees = np.diff(c["offsets"].astype(np.int64))
    assert degrees[0] == k and degrees.max() == k
    assert ref["wall_vertices"][0, 1] == k - 44 and ref["wall_area"][0, 1] > 0
    B.check_against_exact(name, out)


@pytest.mark.parametrize("k,row", [(16, 59), (17, 56), (256, 294)])
def test_a_wall_face_at_the_capacity_of_the_lane_path_and_of_the_serial_path(k, row):
    """the +z wall of RING_BOX cuts site 1's cell in the ring's k-gon: the polygon peaks at exactly k vertices"""
    name = f"ring{k}"
    c, ref, out = B.case(name), B.exact(name), B.host(name)
    assert int(np.diff(c["offsets"].astype(np.int64))[1]) == row
    assert ref["wall_vertices"][1, 5] == k
    B.check_against_exact(name, out)
    assert out["wall_vertices"][1, 5] == k
    at, below = B.host(name, cap=k), B.host(name, cap=k - 1)
    assert at["status"][1] == 0 and below["status"][1] == 1
    assert at["volume"][1] == out["volume"][1] and np.array_equal(at["wall_area"][1], out["wall_area"][1])
    assert np.isnan(below["volume"][1]) and np.isnan(below["wall_area"][1, 5]) and not below["nonempty"][1]


def test_a_257_gon_is_reported_never_a_wrong_number():
    from radfoam_amd import foam

    pts = H._CLOUDS["ring257"]()
    off, adj = foam.delaunay_csr(pts)
    out = B.cell_box(pts, adj, off, B.RING_BOX)
    bad = np.nonzero(out["status"])[0]
    assert len(bad) and (out["status"][bad] == 1).all() and 1 in bad and (bad < 2 + 257).all()
    assert np.isnan(out["volume"][bad]).all() and not out["nonempty"][bad].any()
    roomy = B.cell_box(pts, adj, off, B.RING_BOX, cap=512)
    assert roomy["bad"] == 0 and roomy["wall_vertices"][1, 5] == 257


def test_handed_on_cells_in_several_blocks_of_the_redo_kernel():
    """redo_spread's four 17-rings, whose axis pairs lie in blocks 0, 0, 1 and 3 of the redo kernel: at capacity 16 the
    host build refuses exactly what the lane kernel hands on, and at full capacity the identities hold"""
    c = B.case("redo_spread")
    pairs = np.array(H.REDO_SPREAD_PAIRS)
    assert sorted(set((pairs[:, 0] // 64).tolist())) == [0, 1, 3]
    small = B.host("redo_spread", cap=16)
    assert set(pairs.reshape(-1).tolist()) <= set(np.nonzero(small["status"] == 1)[0].tolist())
    B.check_identities(c, B.host("redo_spread"))


# ---- 5. degenerate positions -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["grid_between", "grid_sites", "grid_bisectors"])
def test_a_grid_whose_walls_pass_between_sites_through_sites_and_along_bisectors(name):
    out = B.host(name)
    assert out["bad"] == 0
    B.check_grid(name, out)


# ---- 6. tiny and malformed inputs ------------------------------------------------------------------------------------

def test_tiny_inputs():
    tiny = H.tiny_inputs()
    box = np.array([-1.0, -2.0, -0.5, 2.0, 1.0, 3.5])
    for name, n in (("n1", 1), ("n2", 2)):                  # empty rows: every cell is the whole box
        pts, off, adj = tiny[name]
        out = B.cell_box(pts, adj, off, box)
        assert out["bad"] == 0 and out["volume"].shape == (n,)
        for a in range(n):
            B.check_whole_box(box, out, a)
    pts, off, adj = tiny["n4"]
    c = dict(points=pts, offsets=off, adjacency=adj, rows=np.repeat(np.arange(4), 3), box=box, name="n4")
    out = B.cell_box(pts, adj, off, box)
    assert out["bad"] == 0 and out["nonempty"].all()
    B.check_identities(c, out)
    a = H.EMPTY_ROW_SITE
    pts, off, adj = tiny["empty_row"]
    cube = np.array([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0])
    full = B.cell_box(*[tiny["empty_row_full"][i] for i in (0, 2, 1)], cube)
    got = B.cell_box(pts, adj, off, cube)
    assert got["bad"] == 0
    B.check_whole_box(cube, got, a)                           # that one cell only: sum V exceeds the box by design
    rest = np.arange(len(pts)) != a
    assert np.array_equal(got["volume"][rest], full["volume"][rest])
    assert abs(full["volume"].sum() - 8.0) <= 8e-9 and got["volume"].sum() > 15.0
    none = B.cell_box(np.zeros((0, 3), dtype=np.float32), np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint32), cube)
    assert none["bad"] == 0 and none["volume"].shape == (0,)


def test_a_malformed_row_is_reported_naming_the_cell():
    c = B.case("uniform400")
    adj = c["adjacency"].copy()
    adj[int(c["offsets"][40])] = 40          # the site itself in its own row
    out = B.cell_box(c["points"], adj, c["offsets"], c["box"])
    assert out["bad"] == 1 and out["status"][40] == 2
    assert np.isnan(out["volume"][40]) and np.isnan(out["wall_area"][40]).all() and not out["nonempty"][40]
    assert np.isnan(out["face_area"][c["rows"] == 40]).all()
    rest = np.arange(len(c["points"])) != 40
    assert np.array_equal(out["volume"][rest], B.host("uniform400")["volume"][rest])
