"""Point gradients of the cells clipped to a box (radfoam.cell_geometry_in_box_grad), the part that runs without a GPU:
how the new kernel file is built, the argument checks, and the numerics of radfoam_amd/csrc/rf_clip_box_grad.hpp,
compiled for the host by tests/host_harness/clip_box_grad_host, against difference quotients of the exact rational boxed
geometry (tests/cell_box_grad_ref.py) and the identities a partition of a fixed box obeys -- the checks
tests/test_gpu_cell_box_grad.py makes on the device, through the same functions.

Measured on the host (spread / max |R| of the reference, then the worst |<grad, delta> - R| / spread over the probes):
  uniform400 5.6e-8 1.4e-5, tight 6.1e-8 1.2e-4, hub58 2.2e-9 1.6e-2, hub59 2.1e-9 0.65, hub64 2.3e-9 1.0e-2,
  hub65 3.1e-9 5.9e-3, ring16_cut 1.8e-9 9.3e-4, ring17_cut 1.9e-8 4.0e-3, redo_spread_cut 4.0e-10 1.0e-2 (the worst
  ratios are on the single-coordinate probes, whose spread is 1e-13 .. 1e-11).
The first-moment partition (check 2), max |grad| / max |grad of the grad_centroid half|: at most 1.8e-16 (wide); the
agreement with cell_geometry_grad on wide: 348 of 400 cells qualify."""
import os

import numpy as np
import pytest
import torch

from tests import cell_box_grad_ref as R
from tests.host_harness import clip_box_grad_host as BG
from tests.host_harness import clip_box_host as B
from tests.host_harness import clip_grad_host as HG
from tests.host_harness import clip_host as H


def _fd(name):
    """(case on the 2^-16 grid, host forward)"""
    c = R.case(name)
    return c, BG.host_forward(("fd", name), c)


def _plain(name):
    c = B.case(name)
    return c, B.host(name)


def test_kernel_file_is_built_but_not_part_of_the_source_hash():
    from radfoam_amd import _lib, build

    names = lambda paths: {os.path.basename(p) for p in paths}
    new = {"rf_cell_box_grad.hip", "rf_clip_box_grad.hpp", "radfoam_hip_box_grad.h"}
    assert "rf_cell_box_grad.hip" in names(build.EXTRA_SOURCES)
    assert {"rf_clip_box_grad.hpp", "radfoam_hip_box_grad.h"} <= names(build.EXTRA_HEADERS)
    assert not names(build.SOURCES + build.HEADERS) & new
    lib = _lib.load()
    for name in ("rf_cell_box_grad", "rf_cell_box_grad_workspace_bytes"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)


def test_entry_point_validates_without_a_device():
    from radfoam_amd import _lib

    lib = _lib.load()
    assert lib.rf_cell_box_grad_workspace_bytes(1000) >= 1000
    unit, none = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0), [None] * 7
    assert lib.rf_cell_box_grad(None, 0, None, None, 0, None, *unit, *none, None, 0, None) == 0       # nothing to do
    assert lib.rf_cell_box_grad(None, 5, None, None, 0, None, *unit, *none, None, 0, None) == -1
    assert "null pointer" in _lib.last_error()
    dummy = np.zeros(64).ctypes.data
    for box in ((0.0, 0.0, 0.0, 1.0, 0.0, 1.0), (0.0, 0.0, 0.0, 1.0, float("nan"), 1.0),
                (0.0, 0.0, -float("inf"), 1.0, 1.0, 1.0)):
        assert lib.rf_cell_box_grad(dummy, 5, dummy, dummy, 4, dummy, *box, *([dummy] * 7), dummy, 4096, None) == -1
        assert "lo < hi" in _lib.last_error()
    assert lib.rf_cell_box_grad(dummy, 5, dummy, dummy, 4, dummy, *unit, *([dummy] * 7), dummy, 2, None) == -2
    assert "workspace" in _lib.last_error()


def test_public_names_and_the_order_of_the_argument_checks():
    """the box first (ValueError, the tensors are not even looked at), then the points"""
    import radfoam

    for name in ("cell_geometry_in_box_grad", "differentiable_cell_geometry_in_box"):
        assert name in radfoam.__all__ and callable(getattr(radfoam, name))
    for bad in ((0, 0, 0, 1, 1), (0, 0, 0, 1, 0, 1), (0, 0, 0, 1, float("nan"), 1), torch.zeros(2, 3), "box", None):
        with pytest.raises(ValueError, match="box must"):
            radfoam.cell_geometry_in_box_grad(None, None, None, bad, None, None, None)
        with pytest.raises(ValueError, match="box must"):
            radfoam.differentiable_cell_geometry_in_box(None, None, None, bad)
    pts = torch.zeros(10, 3)
    adj, off = torch.zeros(5, dtype=torch.uint32), torch.zeros(11, dtype=torch.uint32)
    unit = (0, 0, 0, 1, 1, 1)
    with pytest.raises(RuntimeError, match="points must be a float32 CUDA tensor"):
        radfoam.cell_geometry_in_box_grad(pts, adj, off, unit, None, None, None)
    with pytest.raises(RuntimeError, match="points must be a float32 CUDA tensor"):
        radfoam.differentiable_cell_geometry_in_box(pts, adj, off, unit)


# ---- the difference quotients of the exact geometry ------------------------------------------------------------------

def test_the_cases_keep_what_makes_them_seams():
    """from the exact reference and the host forward"""
    for k, gon in ((58, 14), (59, 15), (64, 15), (65, 16)):
        c, out = _fd(f"hub{k}")
        assert int(c["offsets"][1]) == k and np.diff(c["offsets"].astype(np.int64)).max() == k
        assert c["exact"]["wall_vertices"][0, 1] == gon == out["wall_vertices"][0, 1]
        assert (c["exact"]["face_area"][:k] == 0.0).sum() == 6 and (out["face_area"][:k] == 0.0).sum() == 6
        assert c["cells"].sum() == 9 and out["nonempty"][:9].all()
    for k in (16, 17):
        c, out = _fd(f"ring{k}_cut")
        slot = H.slot_of(c, 0, 1)
        assert c["exact"]["face_vertices"][slot] == k == out["face_vertices"][slot]
        uncut = B.cell_box(c["points"], c["adjacency"], c["offsets"], B.RING_BOX[:5] + (5.0,))
        assert uncut["face_vertices"][slot] == k and 0.99 * uncut["face_area"][slot] < out["face_area"][slot] < \
            uncut["face_area"][slot] - 1e-4
        assert out["wall_area"][:2, 1].min() > 0.0                          # the +x wall bounds both cells
    c, out = _fd("redo_spread_cut")
    wide = B.cell_box(c["points"], c["adjacency"], c["offsets"], B.CASES["redo_spread"][1])
    for (a, b), cut in zip(H.REDO_SPREAD_PAIRS, (False, True, False, True)):
        slot = H.slot_of(c, a, b)
        assert out["face_vertices"][slot] == 17 and (out["face_area"][slot] < wide["face_area"][slot] - 1e-4) == cut
    c, out = _fd("tight")
    p = c["points"].astype(np.float64)
    outside = ((p < c["box"][:3]) | (p > c["box"][3:])).any(1)
    assert outside.sum() == 300 and (c["cells"] & outside).sum() >= 5 and c["cells"].sum() == 82
    assert _fd("uniform400")[0]["cells"].sum() == 68


@pytest.mark.parametrize("name", list(R.FD_CASES))
def test_gradient_matches_difference_quotients_of_the_exact_boxed_geometry(name):
    c, out = _fd(name)
    cells = c["cells"]
    assert out["nonempty"][cells].all()
    ref, rec = R.reference(name), R.recorded(name)
    assert np.array_equal(rec["cells"], cells) and np.array_equal(rec["R"], ref["R"])           # the record the GPU
    assert np.array_equal(rec["spread"], ref["spread"]) and np.array_equal(rec["w"], ref["w"])    # tests read
    assert np.array_equal(rec["u"], ref["u"])
    assert all(np.array_equal(a, b) for a, b in zip(rec["directions"], ref["directions"]))
    grad = BG.host_run(c, out, ref["w"], ref["u"])
    R.check_against_reference(name, ref, grad)
    # the same through a capacity that just fits, and a capacity below the face is reported, never a wrong number
    if name in ("ring16_cut", "ring17_cut"):
        k = int(name[4:6])
        args = (c["points"], c["adjacency"], c["offsets"], c["box"], out, ref["w"], ref["u"])
        fits = BG.cell_box_grad(*args, cap=k)
        assert (fits["status"][:2] == 0).all() and np.array_equal(fits["grad"][:2], grad[:2])
        small = BG.cell_box_grad(*args, cap=k - 1)
        assert (small["status"][:2] == 1).all() and np.isnan(small["grad"][:2]).all()
        ok = small["status"] == 0
        assert np.array_equal(small["grad"][ok], grad[ok])


def test_handed_on_rows_in_several_blocks_of_the_redo_kernel():
    """redo_spread_cut at capacity 16: the host build refuses the eight axis sites, cut or not, whose rows lie in blocks
    0, 1 and 3 of the redo kernel"""
    c, out = _fd("redo_spread_cut")
    pairs = np.array(H.REDO_SPREAD_PAIRS)
    assert sorted(set((pairs.reshape(-1) // 64).tolist())) == [0, 1, 3]
    gv, gc = BG.unit_upstreams(out)
    small = BG.cell_box_grad(c["points"], c["adjacency"], c["offsets"], c["box"], out, gv, gc, cap=16)
    assert set(pairs.reshape(-1).tolist()) <= set(np.nonzero(small["status"] == 1)[0].tolist())
    full = BG.host_run(c, out, gv, gc)
    ok = small["status"] == 0
    assert np.array_equal(small["grad"][ok], full[ok]) and np.isfinite(full).all()


# ---- checks without a reference --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["uniform400", "tight", "wide", "disjoint", "offset", "grid_bisectors"])
def test_a_constant_volume_upstream_has_a_gradient_of_exactly_zero(name):
    """checks 1 and 7"""
    c, out = _plain(name)
    BG.check_partition_volume(c, out, BG.host_run)
    gv, gc = BG.unit_upstreams(out)
    assert np.isfinite(BG.host_run(c, out, gv, gc)).all()


@pytest.mark.parametrize("name", ["uniform400", "tight", "wide", "offset", "disjoint"])
def test_the_first_moment_of_the_partition_is_fixed(name):
    c, out = _plain(name)
    BG.check_partition_moment(c, out, BG.host_run)


@pytest.mark.parametrize("name", ["tight", "disjoint"])
def test_non_finite_upstreams_on_empty_cells_do_not_leak(name):
    c, out = _plain(name)
    BG.check_empty_cells_are_ignored(c, out, BG.host_run, least=100)


@pytest.mark.parametrize("name", ["uniform400", "tight", "offset"])
def test_none_is_zero_and_the_two_upstreams_add(name):
    c, out = _plain(name)
    BG.check_none_and_linearity(c, out, BG.host_run)


def test_cells_that_touch_no_wall_agree_with_cell_geometry_grad():
    c, out = _plain("wide")
    geo = B.host_geometry("uniform400")
    plain = lambda gv, gc: HG.cell_geometry_grad(c["points"], c["adjacency"], c["offsets"], geo, gv, gc)["grad"]
    BG.check_agreement(c, out, out["wall_area"], geo["bounded"], BG.host_run, plain)


def test_tiny_inputs():
    for name, c in BG.tiny_cases().items():
        out = B.cell_box(c["points"], c["adjacency"], c["offsets"], c["box"])
        assert out["bad"] == 0
        BG.check_tiny(c, out, BG.host_run)
    cube = np.array([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0])
    pts, off, adj = np.zeros((0, 3), dtype=np.float32), np.zeros(1, dtype=np.uint32), np.zeros(0, dtype=np.uint32)
    none = BG.cell_box_grad(pts, adj, off, cube, B.cell_box(pts, adj, off, cube), None, None)
    assert none["bad"] == 0 and none["grad"].shape == (0, 3)
    # a cloud one of whose rows is empty: that row is zero, the rest finite
    pts, off, adj = H.tiny_inputs()["empty_row"]
    c = dict(points=pts, offsets=off, adjacency=adj, box=cube)
    out = B.cell_box(pts, adj, off, cube)
    grad = BG.host_run(c, out, *BG.unit_upstreams(out))
    assert np.isfinite(grad).all() and (grad[H.EMPTY_ROW_SITE] == 0.0).all() and np.abs(grad).max() > 0.0


def test_a_257_gon_is_reported_never_a_wrong_number():
    """the ring face of sites 0 and 1, kept whole by the box: the forward refuses the cloud, so the row's status is read
    with a made-up geometry"""
    from radfoam_amd import foam

    pts = H._CLOUDS["ring257"]()
    off, adj = foam.delaunay_csr(pts)
    n = len(pts)
    geo = dict(volume=np.ones(n), centroid=pts.astype(np.float64), nonempty=np.ones(n, dtype=bool))
    got = BG.cell_box_grad(pts, adj, off, B.RING_BOX[:5] + (5.0,), geo, np.ones(n), None)
    bad = np.nonzero(got["status"])[0]
    assert len(bad) and (got["status"][bad] == 1).all() and {0, 1} <= set(bad.tolist()) and (bad < 2 + 257).all()
    assert np.isnan(got["grad"][bad]).all() and np.isfinite(np.delete(got["grad"], bad, axis=0)).all()
    roomy = BG.cell_box_grad(pts, adj, off, B.RING_BOX[:5] + (5.0,), geo, np.ones(n), None, cap=512)
    assert roomy["bad"] == 0


def test_a_malformed_row_is_reported_naming_the_cell():
    c, out = _plain("uniform400")
    adj = c["adjacency"].copy()
    adj[int(c["offsets"][40])] = 40          # the site itself in its own row
    gv, gc = BG.unit_upstreams(out)
    got = BG.cell_box_grad(c["points"], adj, c["offsets"], c["box"], out, gv, gc)
    assert got["bad"] == 1 and got["status"][40] == 2 and np.isnan(got["grad"][40]).all()
    rest = np.arange(len(c["points"])) != 40
    assert np.array_equal(got["grad"][rest], BG.host_run(c, out, gv, gc)[rest])
