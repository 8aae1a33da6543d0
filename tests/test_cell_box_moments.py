"""Second moments of the Voronoi cells clipped to a box (radfoam.cell_moments_in_box), the part that runs without a GPU:
how the new kernel file is built, the arguments' validation, the exact rational reference of
tests/cell_box_moments_ref.py checking itself, and the numerics of radfoam_amd/csrc/rf_clip_box_moments.hpp, compiled for
the host by tests/host_harness/clip_box_moments_host, against that reference and the identities a partition of the box
obeys -- the checks tests/test_gpu_cell_box_moments.py makes on the device, through the same functions.

Measured on the host build, worst |d site| / tr Q, |d central| / tr Q against the exact reference (and, without a bar,
|d central| / tr C): see the table of DESIGN 4.24 and the docstring of tests/test_gpu_cell_box_moments.py."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests.host_harness import clip_box_host as B
from tests.host_harness import clip_box_moments_host as BM
from tests.host_harness import clip_host as H
from tests.host_harness import clip_moments_host as M


def _host(name, cap=256):
    out = BM.host(name, cap)
    return B.host(name), out["site"], out["central"]


# ---- 1. the build and the entry point ----------------------------------------------------------------------------------

def test_kernel_file_is_built_but_not_part_of_the_source_hash():
    from radfoam_amd import _lib, build

    names = lambda paths: {os.path.basename(p) for p in paths}
    new = {"rf_cell_box_moments.hip", "rf_clip_box_moments.hpp", "radfoam_hip_box_moments.h"}
    assert "rf_cell_box_moments.hip" in names(build.EXTRA_SOURCES)
    assert {"rf_clip_box_moments.hpp", "radfoam_hip_box_moments.h"} <= names(build.EXTRA_HEADERS)
    assert not names(build.SOURCES + build.HEADERS) & new
    lib = _lib.load()
    for name in ("rf_cell_box_moments", "rf_cell_box_moments_workspace_bytes"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)


def test_entry_point_validates_without_a_device():
    from radfoam_amd import _lib

    lib = _lib.load()
    assert lib.rf_cell_box_moments_workspace_bytes(1000) >= 1000
    unit, none = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0), [None] * 6
    assert lib.rf_cell_box_moments(None, 0, None, None, 0, None, *unit, *none, None, 0, None) == 0      # nothing to do
    assert lib.rf_cell_box_moments(None, 5, None, None, 0, None, *unit, *none, None, 0, None) == -1
    assert "null pointer" in _lib.last_error()
    dummy = (torch.zeros(64, dtype=torch.float64)).numpy().ctypes.data
    for box in ((0.0, 0.0, 0.0, 1.0, 0.0, 1.0), (0.0, 0.0, 0.0, 1.0, float("nan"), 1.0),
                (0.0, 0.0, -float("inf"), 1.0, 1.0, 1.0)):
        assert lib.rf_cell_box_moments(dummy, 5, dummy, dummy, 4, dummy, *box, *([dummy] * 6), dummy, 4096, None) == -1
        assert "lo < hi" in _lib.last_error()
    assert lib.rf_cell_box_moments(dummy, 5, dummy, dummy, 4, dummy, *unit, *([dummy] * 6), dummy, 2, None) == -2
    assert "workspace" in _lib.last_error()


def test_the_box_is_validated_before_anything_else():
    import radfoam

    assert "cell_moments_in_box" in radfoam.__all__ and "BoxedCellMoments" in radfoam.__all__
    assert radfoam.BoxedCellMoments._fields == ("site_moment", "central_moment", "geometry")
    for bad in ((0, 0, 0, 1, 1), (0, 0, 0, 1, 0, 1), (0, 0, 0, 1, float("nan"), 1), torch.zeros(2, 3), "box", None):
        with pytest.raises(ValueError, match="box must"):
            radfoam.cell_moments_in_box(None, None, None, bad, geometry="not looked at")
    with pytest.raises(RuntimeError, match="points must be a float32 CUDA tensor"):
        radfoam.cell_moments_in_box(torch.zeros(4, 3), torch.zeros(0, dtype=torch.int32),
                                    torch.zeros(5, dtype=torch.int32), (0, 0, 0, 1, 1, 1))
    doc = radfoam.cell_moments_in_box.__doc__
    assert "Not differentiable" in doc and "not built yet" in doc


# ---- the exact reference checks itself: Fractions, equality ---------------------------------------------------------------

def test_the_reference_partitions_a_box_exactly():
    """n4's four cells in a box: the sum of their moments about the box's centre, Q_a + V_a (m q^T + q m^T + q q^T) with
    V_a m the exact first moment and q = p_a - centre, is V_box diag(e_k^2 / 12) with zero off-diagonals -- as Fractions"""
    from tests import cell_box_moments_ref as X

    pts, off, adj = H.tiny_inputs()["n4"]
    box = [-1.0, -2.0, -0.5, 2.0, 1.0, 3.5]
    ref = X.exact_moments_in_box(pts, off, adj, box, range(4))
    lo, hi = [Fraction(x) for x in box[:3]], [Fraction(x) for x in box[3:]]
    e = [hi[k] - lo[k] for k in range(3)]
    vbox = e[0] * e[1] * e[2]
    total, volume = [Fraction(0)] * 6, Fraction(0)
    for a in range(4):
        q = [Fraction(float(pts[a, k])) - (lo[k] + hi[k]) / 2 for k in range(3)]
        V, F, Q = ref["volume"][a], ref["first"][a], ref["site"][a]
        assert V > 0
        volume += V
        total = [total[n] + Q[n] + F[i] * q[j] + q[i] * F[j] + V * q[i] * q[j] for n, (i, j) in enumerate(X.PAIRS)]
    assert volume == vbox
    assert total == [vbox * e[0] ** 2 / 12, vbox * e[1] ** 2 / 12, vbox * e[2] ** 2 / 12, 0, 0, 0]


def test_the_reference_on_the_cubes_of_a_grid():
    """grid_between: the interior cells are cubes of side h about their sites: h^5 / 12 on the diagonal, 0 off it, for the
    moment about the site and about the centroid -- as Fractions"""
    from tests import cell_box_moments_ref as X

    c = B.case("grid_between")
    inner = np.nonzero(H.grid_interior())[0]
    assert len(inner) == 64
    ref = X.exact_moments_in_box(c["points"], c["offsets"], c["adjacency"], c["box"], inner)
    h = Fraction(1, 4)
    cube = [h ** 5 / 12] * 3 + [0, 0, 0]
    for a in inner.tolist():
        assert ref["volume"][a] == h ** 3 and ref["first"][a] == [0, 0, 0]
        assert ref["site"][a] == cube and ref["central"][a] == cube


def test_the_reference_works_on_the_cells_of_the_box_tests():
    """the cells are exactly those clip_box_host.exact works on, and its volumes are the same Fractions"""
    for name in ("hub58", "ring17", "disjoint"):
        ours, theirs = BM.exact(name), B.exact(name)
        assert np.array_equal(ours["done"], theirs["done"])
        assert ours["volume"] == theirs["volume"]


# ---- 2. the exact reference ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", BM.EXACT_CASES)
def test_boxed_moments_against_the_exact_reference(name):
    assert BM.host(name)["bad"] == 0
    BM.check_against_exact(name, *_host(name))


# ---- 3. scaling ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,power", [("scaled_small", -10), ("scaled_large", 10)])
def test_a_power_of_two_scales_the_results_bit_for_bit(name, power):
    (_, site, central), (_, base_site, base_central) = _host(name), _host("uniform400")
    f = 2.0 ** (5 * power)
    assert np.array_equal(site, base_site * f) and np.array_equal(central, base_central * f)


# ---- 4. the partition ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", BM.PARTITION_CASES)
def test_the_moments_of_the_cells_add_up_to_the_box(name):
    assert BM.host(name)["bad"] == 0
    BM.check_partition(B.case(name), *_host(name))


def test_handed_on_cells_in_several_blocks_of_the_redo_kernel():
    """redo_spread's four 17-rings, whose axis pairs lie in blocks 0, 0, 1 and 3 of the redo kernel: at capacity 16 the
    host build refuses exactly what the lane kernel hands on"""
    pairs = np.array(H.REDO_SPREAD_PAIRS)
    assert sorted(set((pairs[:, 0] // 64).tolist())) == [0, 1, 3]
    small = BM.host("redo_spread", cap=16)
    refused = np.nonzero(small["status"] == 1)[0]
    assert set(pairs.reshape(-1).tolist()) <= set(refused.tolist())
    assert np.isnan(small["site"][refused]).all() and np.isnan(small["central"][refused]).all()
    rest = small["status"] == 0
    assert np.array_equal(small["site"][rest], BM.host("redo_spread")["site"][rest])


# ---- 5. agreement with cell_moments ------------------------------------------------------------------------------------

def test_cells_that_touch_no_wall_agree_with_cell_moments():
    for name, share in (("wide", 0.25), ("uniform400", None), ("offset", None)):
        c = B.case(name)
        plain_geo = B.host_geometry(B.CASES[name][0])
        plain = M.cell_moments(c["points"], c["adjacency"], c["offsets"], plain_geo)
        assert plain["bad"] == 0
        BM.check_agreement(c, *_host(name), plain_geo["bounded"], plain["site"], plain["central"], share=share)


# ---- 6. seams ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [58, 59])
def test_a_list_of_64_planes_and_one_of_65(k):
    name = f"hub{k}"
    c = B.case(name)
    degrees = np.diff(c["offsets"].astype(np.int64))
    assert degrees[0] == k and degrees.max() == k
    BM.check_against_exact(name, *_host(name))


@pytest.mark.parametrize("k", [16, 17, 256])
def test_a_wall_face_at_the_capacity_of_the_lane_path_and_of_the_serial_path(k):
    """the +z wall of RING_BOX cuts site 1's cell in the ring's k-gon: the polygon peaks at exactly k vertices"""
    name = f"ring{k}"
    geo, site, central = _host(name)
    assert geo["wall_vertices"][1, 5] == k
    BM.check_against_exact(name, geo, site, central)
    at, below = BM.host(name, cap=k), BM.host(name, cap=k - 1)
    assert at["status"][1] == 0 and below["status"][1] == 1
    assert np.array_equal(at["site"][1], site[1]) and np.array_equal(at["central"][1], central[1])
    assert np.isnan(below["site"][1]).all() and np.isnan(below["central"][1]).all()


def test_a_257_gon_is_reported_never_a_wrong_number():
    from radfoam_amd import foam

    pts = H._CLOUDS["ring257"]()
    off, adj = foam.delaunay_csr(pts)
    roomy_geo = B.cell_box(pts, adj, off, B.RING_BOX, cap=512)
    assert roomy_geo["bad"] == 0
    out = BM.cell_box_moments(pts, adj, off, B.RING_BOX, roomy_geo)
    bad = np.nonzero(out["status"])[0]
    assert len(bad) and (out["status"][bad] == 1).all() and 1 in bad and (bad < 2 + 257).all()
    assert np.isnan(out["site"][bad]).all() and np.isnan(out["central"][bad]).all()
    roomy = BM.cell_box_moments(pts, adj, off, B.RING_BOX, roomy_geo, cap=512)
    assert roomy["bad"] == 0 and np.isfinite(roomy["site"]).all()
    c = dict(points=pts, offsets=off, adjacency=adj, box=np.array(B.RING_BOX), name="ring257 at capacity 512")
    BM.check_partition(c, roomy_geo, roomy["site"], roomy["central"])


# ---- 7. degenerate positions -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["grid_between", "grid_sites", "grid_bisectors"])
def test_a_grid_whose_walls_pass_between_sites_through_sites_and_along_bisectors(name):
    assert BM.host(name)["bad"] == 0
    BM.check_grid(name, *_host(name))


# ---- 8. tiny and malformed inputs ------------------------------------------------------------------------------------

def _both(pts, off, adj, box):
    geo = B.cell_box(pts, adj, off, box)
    return geo, BM.cell_box_moments(pts, adj, off, box, geo)


def test_tiny_inputs():
    tiny = H.tiny_inputs()
    box = np.array([-1.0, -2.0, -0.5, 2.0, 1.0, 3.5])
    for name, n in (("n1", 1), ("n2", 2)):                  # empty rows: every cell is the whole box
        pts, off, adj = tiny[name]
        geo, out = _both(pts, off, adj, box)
        assert out["bad"] == 0 and out["site"].shape == (n, 6)
        for a in range(n):
            BM.check_whole_box(box, pts, out["site"], out["central"], a)
    pts, off, adj = tiny["n4"]
    geo, out = _both(pts, off, adj, box)
    assert out["bad"] == 0
    BM.check_partition(dict(points=pts, box=box, name="n4"), geo, out["site"], out["central"])
    a = H.EMPTY_ROW_SITE
    pts, off, adj = tiny["empty_row"]
    cube = np.array([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0])
    _, full = _both(*[tiny["empty_row_full"][i] for i in (0, 1, 2)], cube)
    _, got = _both(pts, off, adj, cube)
    assert got["bad"] == 0 and full["bad"] == 0
    BM.check_whole_box(cube, pts, got["site"], got["central"], a)
    rest = np.arange(len(pts)) != a
    assert np.array_equal(got["site"][rest], full["site"][rest]) and np.array_equal(got["central"][rest], full["central"][rest])
    assert not np.array_equal(got["site"][a], full["site"][a])
    empty = np.zeros((0, 3), dtype=np.float32), np.zeros(1, dtype=np.uint32), np.zeros(0, dtype=np.uint32)
    _, none = _both(*empty, cube)
    assert none["bad"] == 0 and none["site"].shape == (0, 6)


def test_a_malformed_row_is_reported_naming_the_cell():
    c = B.case("uniform400")
    adj = c["adjacency"].copy()
    adj[int(c["offsets"][40])] = 40          # the site itself in its own row
    out = BM.cell_box_moments(c["points"], adj, c["offsets"], c["box"], B.host("uniform400"))
    assert out["bad"] == 1 and out["status"][40] == 2
    assert np.isnan(out["site"][40]).all() and np.isnan(out["central"][40]).all()
    rest = np.arange(len(c["points"])) != 40
    base = BM.host("uniform400")
    assert np.array_equal(out["site"][rest], base["site"][rest]) and np.array_equal(out["central"][rest], base["central"][rest])


def test_an_empty_cell_has_zero_moments_and_no_central_moment():
    """disjoint: 397 of the 400 cells miss the box: site_moment is 0 in all six (a flat cell's may be a few ulps), the
    central moment NaN wherever nonempty is False"""
    geo, site, central = _host("disjoint")
    ne = geo["nonempty"]
    assert ne.sum() == 3 and np.isnan(central[~ne]).all() and np.isfinite(central[ne]).all()
    assert (site[~ne] == 0.0).all(1).sum() >= 300
