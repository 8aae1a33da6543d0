"""Voronoi cells clipped to a box on the GPU (radfoam.cell_geometry_in_box, the kernels of rf_cell_box.hip) through the
checks of tests/test_cell_box.py (tests/host_harness/clip_box_host): the exact rational reference to 1e-9 in units of each
cell's own size, the identities of a partition of the box, agreement with cell_geometry away from the walls, the seams
between the lane-per-face kernel and the serial one, degenerate grids, tiny and malformed inputs.  The device's results
meet the bars themselves; they are not compared with the host build.

hub58's site 0 (58 neighbours + 6 walls = 64 planes) and ring16's site 1 (a 16-gon on the +z wall) stay on the
wave-per-cell kernel; hub59's site 0 (65 planes), ring17's and ring256's axis cells and redo_spread's four pairs (blocks
0, 0, 1 and 3 of the redo kernel) go through the serial one.

Measured on the MI355X, worst |dV| / s^3, |dc| / s, |dA| / s^2 (faces, walls) against the exact reference: uniform400 and
its scalings 4.8e-15 2.2e-15 2.4e-14 1.7e-14, hub58 1.9e-15 8.8e-16 3.3e-15 1.8e-16, hub59 3.4e-16 1.2e-16 4.5e-15 3.6e-16,
ring16 6.7e-15 4.0e-15 1.1e-14 1.2e-14, ring17 9.9e-15 8.4e-15 1.1e-14 2.0e-15, ring256 1.1e-14 1.9e-14 1.9e-14 1.3e-15;
the identities: sum V at most 1.6e-15, symmetry 6.6e-13 (wide), closure 3.4e-10 (hub58), pyramids 1.9e-14 (tight); the GPU
triangulation of 20,000 points: sum V = 8 exactly, closure 2.9e-13."""
import numpy as np
import pytest
import torch

from tests.host_harness import clip_box_host as B
from tests.host_harness import clip_host as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_GPU = {}


def _tensors(points, offsets, adjacency):
    return (torch.from_numpy(points).to(DEV), torch.from_numpy(adjacency.astype(np.int64)).to(DEV).to(torch.uint32),
            torch.from_numpy(offsets.astype(np.int64)).to(DEV).to(torch.uint32))


def _run(t, box) -> dict:
    """the private runner (face_vertices and wall_vertices included) as numpy"""
    from radfoam_amd import geometry

    geo, fv, wv = geometry._run_geometry_in_box(*geometry._prepare(*t), geometry._box_six(box))
    out = {k: getattr(geo, k).cpu().numpy() for k in geo._fields}
    out["face_vertices"], out["wall_vertices"] = fv.cpu().numpy(), wv.cpu().numpy()
    return out


def _device(name) -> dict:
    """a case's tensors and the operator's answer for them as numpy, once"""
    if name not in _GPU:
        import radfoam

        c = B.case(name)
        t = _tensors(c["points"], c["offsets"], c["adjacency"])
        out = _run(t, c["box"])
        geo = radfoam.cell_geometry_in_box(*t, c["box"].tolist())
        assert isinstance(geo, radfoam.BoxedCellGeometry) and geo.nonempty.dtype == torch.bool
        assert geo.volume.dtype == geo.centroid.dtype == geo.face_area.dtype == geo.wall_area.dtype == torch.float64
        for k in geo._fields:                                   # the public call and the runner: the same bits
            assert np.array_equal(getattr(geo, k).cpu().numpy(), out[k], equal_nan=True)
        _GPU[name] = dict(t=t, out=out)
    return _GPU[name]


# ---- 1. the exact reference ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["uniform400", "tight", "wide", "disjoint", "offset", "scaled_small", "scaled_large"])
def test_cells_in_a_box_against_the_exact_reference(name):
    B.check_against_exact(name, _device(name)["out"])


@pytest.mark.parametrize("name,power", [("scaled_small", -10), ("scaled_large", 10)])
def test_a_power_of_two_scales_the_results_bit_for_bit(name, power):
    out, base = _device(name)["out"], _device("uniform400")["out"]
    f = 2.0 ** power
    assert np.array_equal(out["volume"], base["volume"] * f ** 3) and np.array_equal(out["centroid"], base["centroid"] * f)
    assert np.array_equal(out["face_area"], base["face_area"] * f ** 2)
    assert np.array_equal(out["wall_area"], base["wall_area"] * f ** 2)
    assert np.array_equal(out["face_vertices"], base["face_vertices"])


# ---- 2. identities on whole clouds -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["uniform400", "tight", "wide", "disjoint", "offset", "hub58", "hub59", "ring16", "ring17",
                                  "ring256", "redo_spread"])
def test_the_cells_partition_the_box(name):
    B.check_identities(B.case(name), _device(name)["out"])


# ---- 3. agreement with cell_geometry ---------------------------------------------------------------------------------

def test_cells_that_touch_no_wall_agree_with_cell_geometry():
    from radfoam_amd import geometry

    for name, share in (("wide", 0.25), ("uniform400", None), ("offset", None)):
        d = _device(name)
        geo, fv = geometry._run_geometry(*geometry._prepare(*d["t"]))
        plain = dict(volume=geo.volume.cpu().numpy(), centroid=geo.centroid.cpu().numpy(),
                     bounded=geo.bounded.cpu().numpy(), face_area=geo.face_area.cpu().numpy(),
                     face_vertices=fv.cpu().numpy())
        B.check_agreement(B.case(name), d["out"], plain, share=share)


# ---- 4. seams ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [58, 59])
def test_a_list_of_64_planes_on_the_lane_path_and_one_of_65_on_the_serial_path(k):
    name = f"hub{k}"
    c = B.case(name)
    degrees = np.diff(c["offsets"].astype(np.int64))
    assert degrees[0] == k and degrees.max() == k
    out = _device(name)["out"]
    assert out["wall_vertices"][0, 1] == k - 44
    B.check_against_exact(name, out)


@pytest.mark.parametrize("k", [16, 17, 256])
def test_a_wall_face_at_the_capacity_of_the_lane_path_and_of_the_serial_path(k):
    name = f"ring{k}"
    out = _device(name)["out"]
    assert out["wall_vertices"][1, 5] == k
    B.check_against_exact(name, out)


def test_a_257_gon_raises_naming_a_cell_of_the_ring():
    import radfoam
    from radfoam_amd import foam

    pts = H._CLOUDS["ring257"]()
    off, adj = foam.delaunay_csr(pts)
    with pytest.raises(RuntimeError, match=r"cell_geometry_in_box: cell (\d+) is not supported: a face outgrew 256 "
                                           r"vertices") as err:
        radfoam.cell_geometry_in_box(*_tensors(pts, off, adj), B.RING_BOX)
    assert int(str(err.value).split("cell ")[1].split()[0]) < 2 + 257


def test_handed_on_cells_in_several_blocks_of_the_redo_kernel():
    pairs = np.array(H.REDO_SPREAD_PAIRS)
    assert sorted(set((pairs[:, 0] // 64).tolist())) == [0, 1, 3]
    out = _device("redo_spread")["out"]
    assert (out["nonempty"][pairs.reshape(-1)]).all()
    B.check_identities(B.case("redo_spread"), out)


# ---- 5. degenerate positions -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["grid_between", "grid_sites", "grid_bisectors"])
def test_a_grid_whose_walls_pass_between_sites_through_sites_and_along_bisectors(name):
    B.check_grid(name, _device(name)["out"])


# ---- 6. tiny and malformed inputs ------------------------------------------------------------------------------------

def test_tiny_inputs():
    import radfoam

    tiny = H.tiny_inputs()
    box = np.array([-1.0, -2.0, -0.5, 2.0, 1.0, 3.5])
    for name, n in (("n1", 1), ("n2", 2)):                  # empty rows: every cell is the whole box
        out = _run(_tensors(*tiny[name]), box)
        assert out["volume"].shape == (n,)
        for a in range(n):
            B.check_whole_box(box, out, a)
    pts, off, adj = tiny["n4"]
    c = dict(points=pts, offsets=off, adjacency=adj, rows=np.repeat(np.arange(4), 3), box=box, name="n4")
    out = _run(_tensors(pts, off, adj), box)
    assert out["nonempty"].all()
    B.check_identities(c, out)
    a = H.EMPTY_ROW_SITE
    cube = np.array([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0])
    full, got = (_run(_tensors(*tiny[k]), cube) for k in ("empty_row_full", "empty_row"))
    B.check_whole_box(cube, got, a)                           # that one cell only: sum V exceeds the box by design
    rest = np.arange(len(tiny["empty_row"][0])) != a
    assert np.array_equal(got["volume"][rest], full["volume"][rest])
    assert abs(full["volume"].sum() - 8.0) <= 8e-9 and got["volume"].sum() > 15.0
    none = radfoam.cell_geometry_in_box(torch.zeros((0, 3), device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV),
                                        torch.zeros(1, dtype=torch.int32, device=DEV), cube)
    assert none.volume.shape == (0,) and none.centroid.shape == (0, 3) and none.wall_area.shape == (0, 6)
    assert none.face_area.shape == (0,) and none.nonempty.dtype == torch.bool


def test_a_malformed_row_raises_naming_the_cell():
    import radfoam

    c, d = B.case("uniform400"), _device("uniform400")
    adj = c["adjacency"].astype(np.int64)
    adj[int(c["offsets"][40])] = 40          # the site itself in its own row
    with pytest.raises(RuntimeError, match=r"cell_geometry_in_box: cell 40 is not supported: its adjacency row is malformed"):
        radfoam.cell_geometry_in_box(d["t"][0], torch.from_numpy(adj).to(DEV), d["t"][2], c["box"])


def test_a_bad_box_raises_before_any_launch():
    import radfoam

    t = _device("uniform400")["t"]
    for bad in ((0, 0, 0, 1, 0, 1), (0, 0, 0, 1, float("nan"), 1), (0, 0, 0, 1, 1), torch.zeros(2, 3, device=DEV)):
        with pytest.raises(ValueError, match="box must"):
            radfoam.cell_geometry_in_box(*t, bad)


# ---- 7. GPU only -------------------------------------------------------------------------------------------------------

def test_index_dtypes_box_forms_and_repeat_runs_give_the_same_bits():
    import radfoam

    d = _device("ring17")
    t, out, box = d["t"], d["out"], B.case("ring17")["box"]
    same = lambda geo: all(np.array_equal(getattr(geo, k).cpu().numpy(), out[k], equal_nan=True) for k in geo._fields)
    assert same(radfoam.cell_geometry_in_box(*t, box))                                          # two calls
    assert same(radfoam.cell_geometry_in_box(*t, torch.from_numpy(box).reshape(2, 3).to(DEV)))     # a [2,3] tensor
    for dtype in (torch.int32, torch.int64):                                                    # next to uint32
        assert same(radfoam.cell_geometry_in_box(t[0], t[1].to(dtype), t[2].to(dtype), box))


def test_the_gpu_triangulation_feeds_straight_in():
    """20,000 uniform points, the GPU's own CSR, in [-1,1]^3: |sum V - 8| <= 8e-9 and the identities of check 2"""
    from radfoam_amd.triangulation import Triangulation

    gen = torch.Generator(device="cpu").manual_seed(0)
    start = (torch.rand((20000, 3), generator=gen) * 2.0 - 1.0).to(DEV)
    tri = Triangulation(start)
    points = start[tri.permutation().to(torch.int64)].contiguous()
    adj, off = tri.point_adjacency(), tri.point_adjacency_offsets()
    assert adj.dtype == torch.uint32
    box = np.array([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0])
    out = _run((points, adj, off), box)
    o = off.to(torch.int64).cpu().numpy()
    c = dict(points=points.cpu().numpy(), offsets=o, adjacency=adj.to(torch.int64).cpu().numpy(),
             rows=np.repeat(np.arange(20000), np.diff(o)), box=box, name="triangulation 20000")
    assert out["nonempty"].all() and abs(out["volume"].sum() - 8.0) <= 8e-9
    B.check_identities(c, out)


def test_the_example_moves_every_site_and_keeps_the_partition():
    from examples import foam_lloyd_box as L

    rows = L.run(num_points=2000, steps=3, device=DEV, quiet=True)
    assert len(rows) == 4
    for moved, ratio, spread in rows[:-1]:
        assert moved == 1.0 and abs(ratio - 1.0) <= 1e-9
    assert abs(rows[-1][1] - 1.0) <= 1e-9 and rows[-1][2] < rows[0][2]
