"""Point gradients of the second moments of the cells clipped to a box (radfoam.cell_moments_in_box_grad), the part that
runs without a GPU: how the new kernel file is built, the argument checks, and the numerics of
radfoam_amd/csrc/rf_clip_box_moments_grad.hpp, compiled for the host by tests/host_harness/clip_box_moments_grad_host,
against difference quotients of the exact rational boxed moments (tests/cell_box_moments_grad_ref.py, all four upstreams
at once) and the closed forms and identities of a partition of a fixed box -- the checks
tests/test_gpu_cell_box_moments_grad.py makes on the device, through the same functions.

Measured on the host (spread / max |R| of the reference, then the worst |<grad, delta> - R| / spread over the probes; no
probe needed the floor 1e-9 max |R|):
  uniform400 1.3e-7 4.7e-6, tight 3.7e-8 1.7e-5, hub58 1.0e-8 8.9e-4, hub59 1.9e-9 1.4e-2, hub64 9.8e-9 2.6e-3,
  hub65 6.4e-9 3.3e-2, ring16_cut 1.3e-8 2.8e-3, ring17_cut 1.3e-8 1.7e-3, redo_spread_cut 8.4e-10 3.2e-3; against
  max |R| the misses are 1e-14 .. 6e-13.
Without a reference, worst ratios against the bar 1e-9: the CVT closed form 1.8e-13 (tight), the partition 9.3e-16
(disjoint), the central path 1.0e-11 (tight), fusion 3.6e-14 (tight); against cell_moments_grad on wide 2.3e-12 (348 of
400 cells qualify; bar 2e-9)."""
import os

import numpy as np
import pytest
import torch

from tests import cell_box_moments_grad_ref as R
from tests.host_harness import clip_box_host as B
from tests.host_harness import clip_box_moments_grad_host as MG
from tests.host_harness import clip_host as H


def _fd(name):
    """(case on the 2^-16 grid, host forward)"""
    c = R.case(name)
    return c, MG.host_forward(("fd", name), c)


def _plain(name):
    c = B.case(name)
    return c, B.host(name)


def test_kernel_file_is_built_but_not_part_of_the_source_hash():
    from radfoam_amd import _lib, build

    names = lambda paths: {os.path.basename(p) for p in paths}
    new = {"rf_cell_box_moments_grad.hip", "rf_clip_box_moments_grad.hpp", "radfoam_hip_box_moments_grad.h"}
    assert "rf_cell_box_moments_grad.hip" in names(build.EXTRA_SOURCES)
    assert {"rf_clip_box_moments_grad.hpp", "radfoam_hip_box_moments_grad.h"} <= names(build.EXTRA_HEADERS)
    assert not names(build.SOURCES + build.HEADERS) & new
    lib = _lib.load()
    for name in ("rf_cell_box_moments_grad", "rf_cell_box_moments_grad_workspace_bytes"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)


def test_entry_point_validates_without_a_device():
    from radfoam_amd import _lib

    lib = _lib.load()
    assert lib.rf_cell_box_moments_grad_workspace_bytes(1000) >= 1000
    unit, none = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0), [None] * 9
    assert lib.rf_cell_box_moments_grad(None, 0, None, None, 0, None, *unit, *none, None, 0, None) == 0   # nothing to do
    assert lib.rf_cell_box_moments_grad(None, 5, None, None, 0, None, *unit, *none, None, 0, None) == -1
    assert "null pointer" in _lib.last_error()
    dummy = np.zeros(64).ctypes.data
    for box in ((0.0, 0.0, 0.0, 1.0, 0.0, 1.0), (0.0, 0.0, 0.0, 1.0, float("nan"), 1.0),
                (0.0, 0.0, -float("inf"), 1.0, 1.0, 1.0)):
        assert lib.rf_cell_box_moments_grad(dummy, 5, dummy, dummy, 4, dummy, *box, *([dummy] * 9), dummy, 4096,
                                            None) == -1
        assert "lo < hi" in _lib.last_error()
    assert lib.rf_cell_box_moments_grad(dummy, 5, dummy, dummy, 4, dummy, *unit, *([dummy] * 9), dummy, 2, None) == -2
    assert "workspace" in _lib.last_error()


def test_public_names_and_the_order_of_the_argument_checks():
    """the box first (ValueError, the tensors are not even looked at), then the points"""
    import radfoam

    for name in ("cell_moments_in_box_grad", "differentiable_cell_moments_in_box"):
        assert name in radfoam.__all__ and callable(getattr(radfoam, name))
    for bad in ((0, 0, 0, 1, 1), (0, 0, 0, 1, 0, 1), (0, 0, 0, 1, float("nan"), 1), torch.zeros(2, 3), "box", None):
        with pytest.raises(ValueError, match="box must"):
            radfoam.cell_moments_in_box_grad(None, None, None, bad, None)
        with pytest.raises(ValueError, match="box must"):
            radfoam.differentiable_cell_moments_in_box(None, None, None, bad)
    pts = torch.zeros(10, 3)
    adj, off = torch.zeros(5, dtype=torch.uint32), torch.zeros(11, dtype=torch.uint32)
    unit = (0, 0, 0, 1, 1, 1)
    with pytest.raises(RuntimeError, match="points must be a float32 CUDA tensor"):
        radfoam.cell_moments_in_box_grad(pts, adj, off, unit, None)
    with pytest.raises(RuntimeError, match="points must be a float32 CUDA tensor"):
        radfoam.differentiable_cell_moments_in_box(pts, adj, off, unit)


# ---- 1. the difference quotients of the exact boxed moments ------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.FD_CASES))
def test_gradient_matches_difference_quotients_of_the_exact_boxed_moments(name):
    """one random probe and every seam probe computed afresh must equal the record bit for bit; the host build meets the
    bar on every recorded probe"""
    c, out = _fd(name)
    rec = R.recorded(name)
    assert np.array_equal(rec["cells"], c["cells"]) and out["nonempty"][c["cells"]].all()
    for got, want in zip(R.upstreams(c, c["cells"]), (rec[k] for k in ("A", "B", "w", "u"))):
        assert np.array_equal(got, want)
    for index in [0] + list(range(R.PROBES, len(rec["R"]))):
        fresh = R.probe(name, index)
        assert fresh[0] == rec["R"][index] and fresh[1] == rec["spread"][index]
    print(f"{name}: {c['cells'].sum()} cells in L, reference spread / max |R| = {rec['worst']:.3g}")
    assert rec["worst"] <= R.REFERENCE_SPREAD
    grad = MG.host_run(c, out, rec["A"], rec["B"], rec["w"], rec["u"])
    R.check_against_reference(name, rec, grad)
    # (h) the same through a capacity that just fits, and a capacity below the face is reported, never a wrong number
    if name in ("ring16_cut", "ring17_cut"):
        k = int(name[4:6])
        args = (c["points"], c["adjacency"], c["offsets"], c["box"], out, rec["A"], rec["B"], rec["w"], rec["u"])
        fits = MG.cell_box_moments_grad(*args, cap=k)
        assert (fits["status"][:2] == 0).all() and np.array_equal(fits["grad"][:2], grad[:2])
        small = MG.cell_box_moments_grad(*args, cap=k - 1)
        assert (small["status"][:2] == 1).all() and np.isnan(small["grad"][:2]).all()
        ok = small["status"] == 0
        assert np.array_equal(small["grad"][ok], grad[ok])


def test_handed_on_rows_in_several_blocks_of_the_redo_kernel():
    """(h) redo_spread_cut at capacity 16: the host build refuses the eight axis sites, cut or not, whose rows lie in
    blocks 0, 1 and 3 of the redo kernel"""
    c, out = _fd("redo_spread_cut")
    pairs = np.array(H.REDO_SPREAD_PAIRS)
    assert sorted(set((pairs.reshape(-1) // 64).tolist())) == [0, 1, 3]
    ups = MG.unit_upstreams(out)
    small = MG.cell_box_moments_grad(c["points"], c["adjacency"], c["offsets"], c["box"], out, *ups, cap=16)
    assert set(pairs.reshape(-1).tolist()) <= set(np.nonzero(small["status"] == 1)[0].tolist())
    full = MG.host_run(c, out, *ups)
    ok = small["status"] == 0
    assert np.array_equal(small["grad"][ok], full[ok]) and np.isfinite(full).all()


# ---- 2. closed forms and identities, no reference ------------------------------------------------------------------------

@pytest.mark.parametrize("name", MG.PLAIN_CASES)
def test_the_trace_upstream_gives_the_cvt_gradient_on_every_nonempty_cell(name):
    """(a)"""
    c, out = _plain(name)
    MG.check_cvt(c, out, MG.host_run)


def test_the_cvt_gradient_is_finite_where_walls_coincide_with_bisectors():
    """(a) on grid_bisectors"""
    c, out = _plain("grid_bisectors")
    MG.check_cvt(c, out, MG.host_run, finite_only=True)


@pytest.mark.parametrize("name", MG.PLAIN_CASES)
def test_the_second_moment_of_the_partition_is_fixed(name):
    """(b), with the direct terms autograd would add formed by hand"""
    c, out = _plain(name)
    MG.check_partition(c, out, MG.host_run)


@pytest.mark.parametrize("name", MG.PLAIN_CASES)
def test_the_central_path_equals_the_site_path_minus_the_shift(name):
    """(c), with the direct terms autograd would add formed by hand"""
    c, out = _plain(name)
    MG.check_central_path(c, out, MG.host_run)


@pytest.mark.parametrize("name", MG.PLAIN_CASES)
def test_the_fused_call_is_the_sum_of_its_halves_and_none_is_zero(name):
    """(d)"""
    c, out = _plain(name)
    MG.check_fusion(c, out, MG.host_run, MG.host_geometry_run)


def test_cells_that_touch_no_wall_agree_with_cell_moments_grad():
    """(e)"""
    from tests.host_harness import clip_moments_grad_host as HM

    c, out = _plain("wide")
    geo = B.host_geometry("uniform400")
    plain = lambda gq, gm: HM.cell_moments_grad(c["points"], c["adjacency"], c["offsets"], geo, gq, gm)["grad"]
    MG.check_agreement(c, out, geo["bounded"], MG.host_run, plain)


@pytest.mark.parametrize("name", ["tight", "disjoint"])
def test_non_finite_upstreams_on_empty_cells_do_not_leak(name):
    """(f)"""
    c, out = _plain(name)
    MG.check_empty_cells_are_ignored(c, out, MG.host_run, least=100)


def test_tiny_inputs():
    """(i)"""
    for name, c in MG.tiny_cases().items():
        out = B.cell_box(c["points"], c["adjacency"], c["offsets"], c["box"])
        assert out["bad"] == 0
        MG.check_tiny(c, out, MG.host_run)
    cube = np.array([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0])
    pts, off, adj = np.zeros((0, 3), dtype=np.float32), np.zeros(1, dtype=np.uint32), np.zeros(0, dtype=np.uint32)
    none = MG.cell_box_moments_grad(pts, adj, off, cube, B.cell_box(pts, adj, off, cube), None, None, None, None)
    assert none["bad"] == 0 and none["grad"].shape == (0, 3)
    # a cloud one of whose rows was emptied: that cell is the whole box and has its direct term; with the emptied site's
    # upstreams zeroed, every row that does not list it keeps its bits
    pts, off, adj = H.tiny_inputs()["empty_row"]
    a = H.EMPTY_ROW_SITE
    c = dict(points=pts, offsets=off, adjacency=adj, box=cube)
    out = B.cell_box(pts, adj, off, cube)
    ups = MG.unit_upstreams(out)
    grad = MG.host_run(c, out, *ups)
    centre_minus_p = 0.5 * (cube[:3] + cube[3:]) - pts[a].astype(np.float64)
    want = -2.0 * 8.0 * MG.symmetric(ups[0][a]) @ centre_minus_p
    assert np.isfinite(grad).all() and np.abs(grad[a] - want).max() <= 1e-12 * np.abs(want).max()
    assert (MG.host_run(c, out, None, *ups[1:])[a] == 0.0).all()


def test_an_emptied_row_leaves_every_other_rows_bits():
    """(i) emptying the row of a site whose upstreams are zero and whose cell is flagged empty changes no other row"""
    c, out = _plain("uniform400")
    a = 40
    off = c["offsets"].astype(np.int64)
    lo, hi = int(off[a]), int(off[a + 1])
    adj2 = np.concatenate([c["adjacency"][:lo], c["adjacency"][hi:]])
    off2 = off.copy()
    off2[a + 1:] -= hi - lo
    ups = MG.unit_upstreams(out, seed=6)
    full = MG.host_run(c, out, *ups)
    c2 = dict(c, adjacency=adj2.astype(np.uint32), offsets=off2.astype(np.uint32))
    cut = MG.host_run(c2, out, *ups)
    rest = np.arange(len(c["points"])) != a
    assert np.array_equal(cut[rest], full[rest]) and np.isfinite(cut).all()
    G = MG.symmetric(ups[0][a])
    want = -2.0 * out["volume"][a] * G @ (out["centroid"][a] - c["points"][a].astype(np.float64))
    assert np.abs(cut[a] - want).max() <= 1e-12 * np.abs(want).max()      # the direct term alone is left of row a


def test_a_257_gon_is_reported_never_a_wrong_number():
    """the ring face of sites 0 and 1, kept whole by the box: the forward refuses the cloud, so the row's status is read
    with a made-up geometry"""
    from radfoam_amd import foam

    pts = H._CLOUDS["ring257"]()
    off, adj = foam.delaunay_csr(pts)
    n = len(pts)
    geo = dict(volume=np.ones(n), centroid=pts.astype(np.float64), nonempty=np.ones(n, dtype=bool))
    args = (pts, adj, off, B.RING_BOX[:5] + (5.0,), geo, np.ones((n, 6)), None, np.ones(n), None)
    got = MG.cell_box_moments_grad(*args)
    bad = np.nonzero(got["status"])[0]
    assert len(bad) and (got["status"][bad] == 1).all() and {0, 1} <= set(bad.tolist()) and (bad < 2 + 257).all()
    assert np.isnan(got["grad"][bad]).all() and np.isfinite(np.delete(got["grad"], bad, axis=0)).all()
    assert MG.cell_box_moments_grad(*args, cap=512)["bad"] == 0


def test_a_malformed_row_is_reported_naming_the_cell():
    c, out = _plain("uniform400")
    adj = c["adjacency"].copy()
    adj[int(c["offsets"][40])] = 40          # the site itself in its own row
    ups = MG.unit_upstreams(out)
    got = MG.cell_box_moments_grad(c["points"], adj, c["offsets"], c["box"], out, *ups)
    assert got["bad"] == 1 and got["status"][40] == 2 and np.isnan(got["grad"][40]).all()
    rest = np.arange(len(c["points"])) != 40
    assert np.array_equal(got["grad"][rest], MG.host_run(c, out, *ups)[rest])
