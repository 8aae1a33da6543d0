"""Second moments of the Voronoi cells clipped to a box on the GPU (radfoam.cell_moments_in_box, the kernels of
rf_cell_box_moments.hip) through the checks of tests/test_cell_box_moments.py (tests/host_harness/clip_box_moments_host):
the exact rational reference to 1e-9 of each cell's tr Q, bit-exact power-of-two scaling, the partition of the box's second
moment, agreement with cell_moments away from the walls, the seams between the lane-per-plane kernel and the serial one,
degenerate grids, tiny and malformed inputs, the same bits however it is called, and the GPU triangulation of 4,000
points end to end with the Gaussian export.  The device's results meet the bars themselves; they are not compared with
the host build.

hub58's site 0 (58 neighbours + 6 walls = 64 planes) and ring16's site 1 (a 16-gon on the +z wall) stay on the
wave-per-cell kernel; hub59's site 0 (65 planes), ring17's and ring256's axis cells and redo_spread's four pairs (blocks
0, 0, 1 and 3 of the redo kernel) go through the serial one.

Measured, worst |d site| / tr Q and |d central| / tr Q against the exact reference (bar 1e-9), then, without a bar,
|d central| / tr C; the host build first, the MI355X second:

    case         site, host / MI355X    central, host / MI355X    central / tr C, host / MI355X
    uniform400   5.6e-15 / 5.6e-15      3.9e-15 / 3.9e-15         4.3e-15 / 4.4e-15      (and bit for bit its scalings)
    tight        1.5e-12 / 1.5e-12      2.7e-13 / 2.7e-13         2.9e-10 / 2.8e-10
    wide         2.3e-13 / 2.3e-13      2.0e-13 / 2.0e-13         2.3e-13 / 2.3e-13
    disjoint     4.9e-15 / 5.2e-15      2.0e-15 / 1.7e-15         3.1e-12 / 2.7e-12
    offset       4.3e-15 / 4.3e-15      8.5e-13 / 8.5e-13         1.7e-12 / 1.7e-12
    hub58        1.9e-15 / 1.7e-15      1.9e-15 / 1.7e-15         2.0e-15 / 1.8e-15
    hub59        3.3e-16 / 3.3e-16      3.8e-16 / 3.8e-16         3.8e-16 / 3.8e-16
    ring16       4.6e-15 / 4.6e-15      4.6e-15 / 4.6e-15         7.1e-15 / 7.1e-15
    ring17       4.9e-15 / 4.9e-15      3.8e-15 / 3.8e-15         5.9e-15 / 5.9e-15
    ring256      8.9e-15 / 8.9e-15      4.8e-15 / 4.8e-15         7.5e-15 / 7.5e-15

tight's worst cells are the slivers the box cuts off cells whose sites lie outside it; there V m m^T cancels against Q and
the covariance keeps three digits fewer than the moments do.  The partition identity: at most 1.0e-14 (disjoint), 4,000
points triangulated on the GPU 1.0e-15.
"""
import numpy as np
import pytest
import torch

from tests.host_harness import clip_box_host as B
from tests.host_harness import clip_box_moments_host as BM
from tests.host_harness import clip_host as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_GPU = {}


def _tensors(points, offsets, adjacency):
    return (torch.from_numpy(points).to(DEV), torch.from_numpy(adjacency.astype(np.int64)).to(DEV).to(torch.uint32),
            torch.from_numpy(offsets.astype(np.int64)).to(DEV).to(torch.uint32))


def _numpy(mo) -> tuple:
    """a BoxedCellMoments as (geo dict, site, central) in numpy"""
    geo = {k: getattr(mo.geometry, k).cpu().numpy() for k in mo.geometry._fields}
    return geo, mo.site_moment.cpu().numpy(), mo.central_moment.cpu().numpy()


def _run(t, box) -> tuple:
    import radfoam

    mo = radfoam.cell_moments_in_box(*t, box)
    assert isinstance(mo, radfoam.BoxedCellMoments) and isinstance(mo.geometry, radfoam.BoxedCellGeometry)
    assert mo.site_moment.dtype == mo.central_moment.dtype == torch.float64 and not mo.site_moment.requires_grad
    return _numpy(mo)


def _device(name) -> dict:
    """a case's tensors and the operator's answer for them as numpy (geo, site, central), once"""
    if name not in _GPU:
        c = B.case(name)
        t = _tensors(c["points"], c["offsets"], c["adjacency"])
        _GPU[name] = dict(t=t, out=_run(t, c["box"].tolist()))
    return _GPU[name]


# ---- 2. the exact reference ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", BM.EXACT_CASES)
def test_boxed_moments_against_the_exact_reference(name):
    BM.check_against_exact(name, *_device(name)["out"])


# ---- 3. scaling ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,power", [("scaled_small", -10), ("scaled_large", 10)])
def test_a_power_of_two_scales_the_results_bit_for_bit(name, power):
    (_, site, central), (_, base_site, base_central) = _device(name)["out"], _device("uniform400")["out"]
    f = 2.0 ** (5 * power)
    assert np.array_equal(site, base_site * f) and np.array_equal(central, base_central * f)


# ---- 4. the partition ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", BM.PARTITION_CASES)
def test_the_moments_of_the_cells_add_up_to_the_box(name):
    BM.check_partition(B.case(name), *_device(name)["out"])


def test_handed_on_cells_in_several_blocks_of_the_redo_kernel():
    pairs = np.array(H.REDO_SPREAD_PAIRS)
    assert sorted(set((pairs[:, 0] // 64).tolist())) == [0, 1, 3]
    geo, site, central = _device("redo_spread")["out"]
    handed = pairs.reshape(-1)
    assert geo["nonempty"][handed].all() and np.isfinite(site[handed]).all() and np.isfinite(central[handed]).all()
    assert (site[handed, :3] > 0).all()
    BM.check_partition(B.case("redo_spread"), geo, site, central)


# ---- 5. agreement with cell_moments ------------------------------------------------------------------------------------

def test_cells_that_touch_no_wall_agree_with_cell_moments():
    import radfoam

    for name, share in (("wide", 0.25), ("uniform400", None), ("offset", None)):
        d = _device(name)
        plain = radfoam.cell_moments(*d["t"])
        BM.check_agreement(B.case(name), *d["out"], plain.geometry.bounded.cpu().numpy(), plain.site_moment.cpu().numpy(),
                           plain.central_moment.cpu().numpy(), share=share)


# ---- 6. seams ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [58, 59])
def test_a_list_of_64_planes_on_the_lane_path_and_one_of_65_on_the_serial_path(k):
    name = f"hub{k}"
    c = B.case(name)
    degrees = np.diff(c["offsets"].astype(np.int64))
    assert degrees[0] == k and degrees.max() == k
    BM.check_against_exact(name, *_device(name)["out"])


@pytest.mark.parametrize("k", [16, 17, 256])
def test_a_wall_face_at_the_capacity_of_the_lane_path_and_of_the_serial_path(k):
    """the +z wall cuts site 1's cell in the ring's k-gon (tests/test_gpu_cell_box.py counts its vertices)"""
    name = f"ring{k}"
    geo, site, central = _device(name)["out"]
    assert geo["wall_area"][1, 5] > 0 and np.isfinite(central[1]).all()
    BM.check_against_exact(name, geo, site, central)


def test_a_257_gon_raises_naming_a_cell_of_the_ring():
    """with geometry=None cell_geometry_in_box raises first; given a geometry (the host build's, at capacity 512) this
    operator's own redo kernel does"""
    import radfoam
    from radfoam_amd import foam

    pts = H._CLOUDS["ring257"]()
    off, adj = foam.delaunay_csr(pts)
    t = _tensors(pts, off, adj)
    with pytest.raises(RuntimeError, match=r"cell_geometry_in_box: cell (\d+) is not supported: a face outgrew 256 "
                                           r"vertices"):
        radfoam.cell_moments_in_box(*t, B.RING_BOX)
    roomy = B.cell_box(pts, adj, off, B.RING_BOX, cap=512)
    assert roomy["bad"] == 0
    geo = radfoam.BoxedCellGeometry(*(torch.from_numpy(roomy[k]).to(DEV) for k in radfoam.BoxedCellGeometry._fields))
    with pytest.raises(RuntimeError, match=r"cell_moments_in_box: cell (\d+) is not supported: a face outgrew 256 "
                                           r"vertices") as err:
        radfoam.cell_moments_in_box(*t, B.RING_BOX, geometry=geo)
    assert int(str(err.value).split("cell ")[1].split()[0]) < 2 + 257


# ---- 7. degenerate positions -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["grid_between", "grid_sites", "grid_bisectors"])
def test_a_grid_whose_walls_pass_between_sites_through_sites_and_along_bisectors(name):
    BM.check_grid(name, *_device(name)["out"])


# ---- 8. tiny and malformed inputs ------------------------------------------------------------------------------------

def test_tiny_inputs():
    import radfoam

    tiny = H.tiny_inputs()
    box = np.array([-1.0, -2.0, -0.5, 2.0, 1.0, 3.5])
    for name, n in (("n1", 1), ("n2", 2)):                  # empty rows: every cell is the whole box
        geo, site, central = _run(_tensors(*tiny[name]), box)
        assert site.shape == (n, 6)
        for a in range(n):
            BM.check_whole_box(box, tiny[name][0], site, central, a)
    pts, off, adj = tiny["n4"]
    geo, site, central = _run(_tensors(pts, off, adj), box)
    assert geo["nonempty"].all()
    BM.check_partition(dict(points=pts, box=box, name="n4"), geo, site, central)
    a = H.EMPTY_ROW_SITE
    cube = np.array([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0])
    (_, full_site, full_central), (_, site, central) = (_run(_tensors(*tiny[k]), cube) for k in ("empty_row_full", "empty_row"))
    BM.check_whole_box(cube, tiny["empty_row"][0], site, central, a)
    rest = np.arange(len(tiny["empty_row"][0])) != a
    assert np.array_equal(site[rest], full_site[rest]) and np.array_equal(central[rest], full_central[rest])
    assert not np.array_equal(site[a], full_site[a])
    none = radfoam.cell_moments_in_box(torch.zeros((0, 3), device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV),
                                       torch.zeros(1, dtype=torch.int32, device=DEV), cube)
    assert none.site_moment.shape == (0, 6) and none.central_moment.shape == (0, 6)
    assert none.site_moment.dtype == torch.float64 and none.geometry.volume.shape == (0,)


def test_a_malformed_row_raises_naming_the_cell():
    import radfoam

    c, d = B.case("uniform400"), _device("uniform400")
    adj = c["adjacency"].astype(np.int64)
    adj[int(c["offsets"][40])] = 40          # the site itself in its own row
    bad = torch.from_numpy(adj).to(DEV)
    with pytest.raises(RuntimeError, match=r"cell_geometry_in_box: cell 40 is not supported: its adjacency row is malformed"):
        radfoam.cell_moments_in_box(d["t"][0], bad, d["t"][2], c["box"])
    geo = radfoam.cell_geometry_in_box(*d["t"], c["box"])
    with pytest.raises(RuntimeError, match=r"cell_moments_in_box: cell 40 is not supported: its adjacency row is malformed"):
        radfoam.cell_moments_in_box(d["t"][0], bad, d["t"][2], c["box"], geometry=geo)


def test_a_bad_box_raises_before_any_launch_and_a_geometry_that_does_not_fit_is_refused():
    import radfoam

    c, t = B.case("uniform400"), _device("uniform400")["t"]
    for bad in ((0, 0, 0, 1, 0, 1), (0, 0, 0, 1, float("nan"), 1), (0, 0, 0, 1, 1), torch.zeros(2, 3, device=DEV)):
        with pytest.raises(ValueError, match="box must"):
            radfoam.cell_moments_in_box(*t, bad, geometry="not looked at")
    geo = radfoam.cell_geometry_in_box(*t, c["box"])
    wrong = ("a string", radfoam.cell_geometry(*t),                                     # the type
             geo._replace(volume=geo.volume[:-1]), geo._replace(centroid=geo.centroid[:, :2]),      # the shape
             geo._replace(volume=geo.volume.float()), geo._replace(nonempty=geo.nonempty.to(torch.uint8)),     # the dtype
             geo._replace(centroid=geo.centroid.cpu()))                                  # the device
    for g in wrong:
        with pytest.raises(RuntimeError, match="geometry must be the BoxedCellGeometry"):
            radfoam.cell_moments_in_box(*t, c["box"], geometry=g)


# ---- 9. the same bits --------------------------------------------------------------------------------------------------

def test_a_geometry_index_dtypes_box_forms_and_repeat_runs_give_the_same_bits():
    import radfoam

    d = _device("ring17")
    t, (geo, site, central), box = d["t"], d["out"], B.case("ring17")["box"]

    def same(mo):
        g, s, c = _numpy(mo)
        return (np.array_equal(s, site) and np.array_equal(c, central, equal_nan=True)
                and all(np.array_equal(g[k], geo[k], equal_nan=True) for k in geo))

    assert same(radfoam.cell_moments_in_box(*t, box))                                           # two calls
    given = radfoam.cell_geometry_in_box(*t, box)
    mo = radfoam.cell_moments_in_box(*t, box, geometry=given)                                   # a geometry passed in
    assert same(mo) and mo.geometry is given
    assert same(radfoam.cell_moments_in_box(*t, torch.from_numpy(box).reshape(2, 3).to(DEV)))      # a [2,3] tensor
    for dtype in (torch.int32, torch.int64):                                                    # next to uint32
        assert same(radfoam.cell_moments_in_box(t[0], t[1].to(dtype), t[2].to(dtype), box))


# ---- 10. end to end ------------------------------------------------------------------------------------------------------

def test_the_gpu_triangulation_and_the_gaussian_export(tmp_path):
    """4,000 uniform points, the GPU's own CSR, in [-1,1]^3: every cell non-empty and finite in all twelve, the partition
    identity; the example writes one Gaussian per site with the box and 3,841 without, finite positive scales and unit
    quaternions, and gaussians_from_moments reproduces central / V to 1e-12 of its trace"""
    import radfoam
    from examples import foam_to_gaussians as G
    from radfoam_amd.triangulation import Triangulation

    gen = torch.Generator(device="cpu").manual_seed(0)
    start = (torch.rand((4000, 3), generator=gen) * 2.0 - 1.0).to(DEV)
    tri = Triangulation(start)
    points = start[tri.permutation().to(torch.int64)].contiguous()
    box = np.array([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0])
    mo = radfoam.cell_moments_in_box(points, tri.point_adjacency(), tri.point_adjacency_offsets(), box)
    geo, site, central = _numpy(mo)
    assert geo["nonempty"].all() and np.isfinite(site).all() and np.isfinite(central).all()
    BM.check_partition(dict(points=points.cpu().numpy(), box=box, name="triangulation 4000"), geo, site, central)

    g = G.gaussians_from_moments(mo)
    assert g["cell"].shape == (4000,) and bool((g["scale"] > 0).all()) and bool(torch.isfinite(g["scale"]).all())
    w, x, y, z = g["rotation"].unbind(-1)
    rot = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                       torch.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                       torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)
    cov = rot @ torch.diag_embed(g["scale"] ** 2) @ rot.transpose(1, 2)
    want = G._symmetric(mo.central_moment / mo.geometry.volume[:, None])
    trace = want.diagonal(dim1=1, dim2=2).sum(1)
    assert float(((cov - want).abs().amax((1, 2)) / trace).max()) <= 1e-12

    counts = {}
    for name, arg in (("boxed", box.tolist()), ("plain", None)):
        path = tmp_path / f"{name}.ply"
        written, energy, surrogate = G.run(num_points=4000, out=str(path), device=DEV, quiet=True, box=arg)
        head, body = path.read_bytes().split(b"end_header\n", 1)
        assert f"element vertex {written}".encode() in head
        table = np.frombuffer(body, dtype="<f4").reshape(written, len(G.PLY_FIELDS))
        assert np.isfinite(table).all() and np.abs(np.linalg.norm(table[:, 13:17], axis=1) - 1.0).max() <= 1e-6
        assert 0.0 < surrogate < energy
        counts[name] = (written, energy)
    print(f"Gaussians written: {counts['boxed'][0]} with the box, {counts['plain'][0]} without; CVT energy sum tr "
          f"site_moment: {counts['boxed'][1]:.6g} over all sites, {counts['plain'][1]:.6g} over the bounded cells")
    assert counts["boxed"][0] == 4000 and counts["plain"][0] == 3841
    assert abs(counts["boxed"][1] - float(site[:, :3].sum())) <= 1e-12 * counts["boxed"][1]
