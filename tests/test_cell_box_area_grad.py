"""Point gradients of the face and wall areas of the cells clipped to a box (radfoam.face_area_in_box_grad), the part that
runs without a GPU: how the new kernel file is built, the argument checks, and the numerics of
radfoam_amd/csrc/rf_clip_box_area_grad.hpp, compiled for the host by tests/host_harness/clip_box_area_grad_host, against
difference quotients of the exact rational boxed areas (tests/cell_box_area_grad_ref.py), the identities the areas of a
partition of a fixed box obey and the unboxed operator -- the checks tests/test_gpu_cell_box_area_grad.py makes on the
device, through the same functions.

Measured on the host: see DESIGN.md, "Point gradients of the face and wall areas in a box" (spread / max |R| of the
reference and the worst |<grad, delta> - R| / spread per case)."""
import os

import numpy as np
import pytest
import torch

from tests import cell_box_area_grad_ref as R
from tests.host_harness import clip_area_grad_host as AG
from tests.host_harness import clip_box_area_grad_host as A
from tests.host_harness import clip_box_host as B
from tests.host_harness import clip_host as H


def _fd(name):
    """(case on the 2^-16 grid, host forward)"""
    c = R.case(name)
    return c, A.host_forward(("fd", name), c)


def _plain(name):
    return A.with_rows(B.case(name)), B.host(name)


def test_kernel_file_is_built_but_not_part_of_the_source_hash():
    from radfoam_amd import _lib, build

    names = lambda paths: {os.path.basename(p) for p in paths}
    new = {"rf_cell_box_area_grad.hip", "rf_clip_box_area_grad.hpp", "radfoam_hip_box_area_grad.h"}
    assert "rf_cell_box_area_grad.hip" in names(build.EXTRA_SOURCES)
    assert {"rf_clip_box_area_grad.hpp", "radfoam_hip_box_area_grad.h"} <= names(build.EXTRA_HEADERS)
    assert not names(build.SOURCES + build.HEADERS) & new
    lib = _lib.load()
    for name in ("rf_cell_box_area_grad", "rf_cell_box_area_grad_workspace_bytes"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)


def test_entry_point_validates_without_a_device():
    from radfoam_amd import _lib

    lib = _lib.load()
    assert lib.rf_cell_box_area_grad_workspace_bytes(1000, 7000) >= 1000 + 8 * 7000
    unit, none = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0), [None] * 9
    assert lib.rf_cell_box_area_grad(None, 0, None, None, 0, None, *unit, *none, None, 0, None) == 0    # nothing to do
    assert lib.rf_cell_box_area_grad(None, 5, None, None, 0, None, *unit, *none, None, 0, None) == -1
    assert "null pointer" in _lib.last_error()
    dummy = np.zeros(64).ctypes.data
    for box in ((0.0, 0.0, 0.0, 1.0, 0.0, 1.0), (0.0, 0.0, 0.0, 1.0, float("nan"), 1.0),
                (0.0, 0.0, -float("inf"), 1.0, 1.0, 1.0)):
        assert lib.rf_cell_box_area_grad(dummy, 5, dummy, dummy, 4, dummy, *box, *([dummy] * 9), dummy, 4096, None) == -1
        assert "lo < hi" in _lib.last_error()
    assert lib.rf_cell_box_area_grad(dummy, 5, dummy, dummy, 4, dummy, *unit, *([dummy] * 9), dummy, 2, None) == -2
    assert "workspace" in _lib.last_error()


def test_public_names_and_the_order_of_the_argument_checks():
    """the box first (ValueError, the tensors are not even looked at), then the points"""
    import radfoam

    assert "face_area_in_box_grad" in radfoam.__all__ and callable(radfoam.face_area_in_box_grad)
    for bad in ((0, 0, 0, 1, 1), (0, 0, 0, 1, 0, 1), (0, 0, 0, 1, float("nan"), 1), torch.zeros(2, 3), "box", None):
        with pytest.raises(ValueError, match="box must"):
            radfoam.face_area_in_box_grad(None, None, None, bad, None)
        with pytest.raises(ValueError, match="box must"):
            radfoam.differentiable_cell_geometry_in_box(None, None, None, bad, face_area=True)
    pts = torch.zeros(10, 3)
    adj, off = torch.zeros(5, dtype=torch.uint32), torch.zeros(11, dtype=torch.uint32)
    unit = (0, 0, 0, 1, 1, 1)
    with pytest.raises(RuntimeError, match="points must be a float32 CUDA tensor"):
        radfoam.face_area_in_box_grad(pts, adj, off, unit, None, None, None)
    with pytest.raises(RuntimeError, match="points must be a float32 CUDA tensor"):
        radfoam.differentiable_cell_geometry_in_box(pts, adj, off, unit, face_area=True)


# ---- the difference quotients of the exact areas ---------------------------------------------------------------------

def test_every_case_keeps_a_wall_and_a_wall_cut_face():
    """from the exact base areas: each case keeps at least 90 % of its positive slots and walls (all of them), a wall, and
    a face the box cuts: a kept slot whose exact boxed area is below the host's unboxed area of the same slot"""
    for name in R.FD_CASES:
        c, out = _fd(name)
        b = R.base(name)
        keep_slot, keep_wall = R.kept(name, b)
        assert keep_wall.sum() >= 1 and keep_slot.sum() >= R.KEEP_SHARE * b["positive_slot"].sum()
        assert keep_wall.sum() >= R.KEEP_SHARE * b["positive_wall"].sum()
        free = H.cell_geometry(c["points"], c["adjacency"], c["offsets"])["face_area"]
        s2 = np.cbrt(c["exact"]["volume_f"][c["rows"]]) ** 2
        cut = keep_slot & (b["slot_area"] < free - 1e-6 * s2)
        print(f"{name}: {keep_slot.sum()} slots ({cut.sum()} cut by a wall) and {keep_wall.sum()} walls in L")
        assert cut.sum() >= 1
        # the forward under test masks what the reference masks
        assert np.array_equal(out["face_area"][c["cells"][c["rows"]]] > 0, b["positive_slot"][c["cells"][c["rows"]]])
        assert np.array_equal(out["wall_area"][c["cells"]] > 0, b["positive_wall"][c["cells"]])


@pytest.mark.parametrize("name", list(R.FD_CASES))
def test_gradient_matches_difference_quotients_of_the_exact_boxed_areas(name):
    c, out = _fd(name)
    ref, rec = R.reference(name), R.recorded(name)
    for k in ("keep_slot", "keep_wall", "g", "gw", "R", "spread"):                   # the record the GPU tests read
        assert np.array_equal(rec[k], ref[k]), k
    assert all(np.array_equal(a, b) for a, b in zip(rec["directions"], ref["directions"]))
    grad = A.host_run(c, out, ref["g"], ref["gw"])
    R.check_against_reference(name, ref, grad)
    # the same through a capacity that just fits, and a capacity below the face is reported, never a wrong number
    if name in ("ring16_cut", "ring17_cut"):
        k = int(name[4:6])
        args = (c["points"], c["adjacency"], c["offsets"], c["box"], out, ref["g"], ref["gw"])
        fits = A.cell_box_area_grad(*args, cap=k)
        assert (fits["status"][:2] == 0).all() and np.array_equal(fits["grad"][:2], grad[:2])
        small = A.cell_box_area_grad(*args, cap=k - 1)
        assert (small["status"][:2] == 1).all() and np.isnan(small["grad"][:2]).all()
        ok = small["status"] == 0
        assert np.array_equal(small["grad"][ok], grad[ok])


def test_handed_on_rows_in_several_blocks_of_the_redo_kernel():
    """redo_spread_cut at capacity 16: the host build refuses the eight axis sites, cut or not, whose rows lie in blocks
    0, 1 and 3 of the redo kernel"""
    c, out = _fd("redo_spread_cut")
    pairs = np.array(H.REDO_SPREAD_PAIRS)
    assert sorted(set((pairs.reshape(-1) // 64).tolist())) == [0, 1, 3]
    g, gw = A.unit_upstreams(c, out)
    small = A.cell_box_area_grad(c["points"], c["adjacency"], c["offsets"], c["box"], out, g, gw, cap=16)
    assert set(pairs.reshape(-1).tolist()) <= set(np.nonzero(small["status"] == 1)[0].tolist())
    full = A.host_run(c, out, g, gw)
    ok = small["status"] == 0
    assert np.array_equal(small["grad"][ok], full[ok]) and np.isfinite(full).all()


# ---- checks without a reference --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,exact", [("uniform400", True), ("wide", True), ("offset", True), ("tight", False),
                                        ("disjoint", False), ("grid_bisectors", False)])
def test_a_wall_upstream_constant_down_each_column_has_no_gradient(name, exact):
    c, out = _plain(name)
    A.check_constant_wall_upstream(c, out, A.host_run, exact)


@pytest.mark.parametrize("name", ["uniform400", "tight", "wide"])
def test_the_area_vectors_close_identically_in_the_points(name):
    c, out = _plain(name)
    A.check_closure(c, out, A.host_run)


def test_slots_away_from_the_walls_agree_with_face_area_grad():
    c, out = _plain("wide")
    geo = B.host_geometry("uniform400")
    plain = lambda g: AG.face_area_grad(c["points"], c["adjacency"], c["offsets"], geo["face_area"], g)["grad"]
    A.check_agreement(c, out, geo, A.host_run, plain)


@pytest.mark.parametrize("name", ["tight", "disjoint"])
def test_non_finite_upstreams_on_empty_cells_do_not_leak(name):
    c, out = _plain(name)
    A.check_empty_cells_are_ignored(c, out, A.host_run, least=100)


@pytest.mark.parametrize("name", ["uniform400", "tight", "offset"])
def test_none_is_zero_and_the_two_upstreams_add(name):
    c, out = _plain(name)
    A.check_none_and_additivity(c, out, A.host_run)


def test_degenerate_clouds():
    c, out = _plain("grid_bisectors")
    assert np.isfinite(A.host_run(c, out, *A.unit_upstreams(c, out))).all()
    for name, c in A.tiny_cases().items():
        out = B.cell_box(c["points"], c["adjacency"], c["offsets"], c["box"])
        assert out["bad"] == 0
        A.check_tiny(c, out, A.host_run)
    cube = np.array([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0])
    pts, off, adj = np.zeros((0, 3), dtype=np.float32), np.zeros(1, dtype=np.uint32), np.zeros(0, dtype=np.uint32)
    none = A.cell_box_area_grad(pts, adj, off, cube, B.cell_box(pts, adj, off, cube), None, None)
    assert none["bad"] == 0 and none["grad"].shape == (0, 3)
    pts, off, adj = H.tiny_inputs()["empty_row"]
    c = A.with_rows(dict(points=pts, offsets=off, adjacency=adj, box=cube))
    out = B.cell_box(pts, adj, off, cube)
    grad = A.host_run(c, out, *A.unit_upstreams(c, out))
    assert np.isfinite(grad).all() and (grad[H.EMPTY_ROW_SITE] == 0.0).all() and np.abs(grad).max() > 0.0


def test_a_257_gon_is_reported_never_a_wrong_number():
    """the ring face of sites 0 and 1, kept whole by the box: the forward refuses the cloud, so the row's status is read
    with a made-up geometry"""
    from radfoam_amd import foam

    pts = H._CLOUDS["ring257"]()
    off, adj = foam.delaunay_csr(pts)
    n, e = len(pts), len(adj)
    geo = dict(nonempty=np.ones(n, dtype=bool), face_area=np.ones(e), wall_area=np.ones((n, 6)))
    box = B.RING_BOX[:5] + (5.0,)
    got = A.cell_box_area_grad(pts, adj, off, box, geo, np.ones(e), None)
    bad = np.nonzero(got["status"])[0]
    assert len(bad) and (got["status"][bad] == 1).all() and {0, 1} <= set(bad.tolist()) and (bad < 2 + 257).all()
    assert np.isnan(got["grad"][bad]).all() and np.isfinite(np.delete(got["grad"], bad, axis=0)).all()
    assert A.cell_box_area_grad(pts, adj, off, box, geo, np.ones(e), None, cap=512)["bad"] == 0


def test_a_malformed_row_is_reported_naming_the_cell():
    c, out = _plain("uniform400")
    adj = c["adjacency"].copy()
    adj[int(c["offsets"][40])] = 40          # the site itself in its own row
    g, gw = A.unit_upstreams(c, out)
    got = A.cell_box_area_grad(c["points"], adj, c["offsets"], c["box"], out, g, gw)
    assert got["bad"] == 1 and got["status"][40] == 2 and np.isnan(got["grad"][40]).all()
    assert np.isfinite(np.delete(got["grad"], 40, axis=0)).all()


def test_every_labelled_edge_lies_on_the_plane_of_its_label():
    """check 10 on the cells of L of tight and of the cut cases, and on every cell of uniform400 in its box.  The unjittered
    grid is left out on purpose: its faces of positive area that should be points are rounding slivers some 1e-17 across,
    less than an ulp of their own coordinates, and "the face's size" is no unit there; that the labelled step reproduces
    the unlabelled vertices bit for bit is still asserted on it."""
    for name in ("tight", "hub65", "ring17_cut"):
        c, out = _fd(name)
        voronoi, wall = A.check_labels(c, out, np.nonzero(c["cells"])[0].tolist())
        print(f"{name}: {voronoi} Voronoi and {wall} wall edges on their planes")
        assert voronoi > 0 and wall > 0
    c, out = _plain("uniform400")
    voronoi, wall = A.check_labels(c, out, range(len(c["points"])))
    assert voronoi > 0 and wall > 0
    c, out = _plain("grid_bisectors")
    off = c["offsets"].astype(np.int64)
    for a in range(len(c["points"])):
        for i in range(int(off[a + 1] - off[a])):
            assert A.labelled_polygon(c, a, i)[2]
