"""Second moments of the Voronoi cells on the GPU (radfoam.cell_moments) against the exact rational reference
(tests/cell_moments_ref.py) on the kernel's seams, to the bar of tests/test_cell_moments.py: |delta| <= 1e-9 tr Q_exact[a]
on each of the twelve numbers of every cell the reference and the code call bounded (clip_moments_host.check_against_exact;
the worst ratio per case is printed).

ring16's axis cells and hub64's row 0 stay on the wave-per-cell kernel; ring17's axis cells (17-gons), hub65's and hub200's
row 0 (more than 64 faces), redo_spread's four pairs (blocks 0, 0, 1 and 3 of the redo kernel) and ring256's axis cells
(the serial capacity) go through the serial one.

Measured on the MI355X, worst |d site| / tr Q and |d central| / tr Q: ring16 2.9e-15 2.9e-15, ring17 6.7e-15 4.1e-15,
ring256 (axis cells) 9.8e-15 2.5e-15, hub64 9.7e-15 2.0e-15, hub65 6.1e-15 2.3e-15, hub200 2.3e-14 3.2e-15,
redo_spread 1.4e-14 1.4e-14, uniform400 1.3e-14 5.7e-15, offset 7.7e-15 8.5e-13, grid 1.0e-15 1.0e-15,
clustered 1.1e-10 6.7e-11; the GPU triangulation of 4,000 points: parallel-axis identity 4.2e-16 of tr site, smallest
eigenvalue of central 6.1e-5 of tr site."""
import numpy as np
import pytest
import torch

from tests.host_harness import clip_host as H
from tests.host_harness import clip_moments_host as HM

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_GPU = {}


def _tensors(points, offsets, adjacency):
    return (torch.from_numpy(points).to(DEV), torch.from_numpy(adjacency.astype(np.int64)).to(DEV).to(torch.uint32),
            torch.from_numpy(offsets.astype(np.int64)).to(DEV).to(torch.uint32))


def _device_case(name):
    """the case's tensors, cell_moments' answer for them and its fields as numpy, once"""
    if name not in _GPU:
        import radfoam

        c = H.case(name)
        t = _tensors(c["points"], c["offsets"], c["adjacency"])
        mo = radfoam.cell_moments(*t)
        n = len(c["points"])
        assert isinstance(mo, radfoam.CellMoments) and isinstance(mo.geometry, radfoam.CellGeometry)
        assert mo.site_moment.dtype == torch.float64 and mo.site_moment.shape == (n, 6)
        assert mo.central_moment.dtype == torch.float64 and mo.central_moment.shape == (n, 6)
        _GPU[name] = (t, mo, dict(site=mo.site_moment.cpu().numpy(), central=mo.central_moment.cpu().numpy(),
                                  bounded=mo.geometry.bounded.cpu().numpy()))
    return _GPU[name]


def _check(name, cells=None):
    out = _device_case(name)[2]
    return HM.check_against_exact(name, out["bounded"], out["site"], out["central"], cells=cells)


@pytest.mark.parametrize("k", [16, 17, 256])
def test_a_k_gon_at_the_capacity_of_the_lane_path_and_of_the_serial_path(k):
    """16 vertices stay in the lane's LDS slot, 17 hand both axis cells on (every other cell stays on the wave path and
    is compared as well), 256 fill the serial path."""
    name = f"ring{k}"
    c = H.case(name)
    assert c["slots"]["vertices"][H.slot_of(c, 0, 1)] == k
    _check(name, cells=[0, 1])
    _check(name)


@pytest.mark.parametrize("k", [64, 65, 200])
def test_a_row_of_64_faces_on_the_wave_path_and_longer_rows_on_the_serial_path(k):
    name = f"hub{k}"
    assert int(H.case(name)["offsets"][1]) == k
    _check(name, cells=[0])
    _check(name)


def test_handed_on_cells_in_several_blocks_of_the_redo_kernel():
    pairs = np.array(H.REDO_SPREAD_PAIRS)
    assert sorted(set((pairs[:, 0] // 64).tolist())) == [0, 1, 3]
    _check("redo_spread", cells=pairs.reshape(-1))
    _check("redo_spread")


@pytest.mark.parametrize("name", ["clustered", "uniform400", "offset", "grid"])
def test_cells_of_very_different_sizes_far_from_the_origin_and_on_a_grid(name):
    _check(name)
    if name == "grid":          # the closed form: h^5 / 12 on the diagonal, 0 off it, site == central
        out, inner = _device_case(name)[2], H.grid_interior()
        h5 = H.GRID_H ** 5 / 12.0
        for key in ("site", "central"):
            assert np.abs(out[key][inner][:, :3] - h5).max() <= 1e-9 * 3 * h5
            assert np.abs(out[key][inner][:, 3:]).max() <= 1e-9 * 3 * h5


@pytest.mark.parametrize("name,power", [("scaled_small", -10), ("scaled_large", 10)])
def test_a_power_of_two_scales_the_moments_bit_for_bit(name, power):
    out, base = _device_case(name)[2], _device_case("uniform400")[2]
    assert np.array_equal(out["bounded"], base["bounded"]) and base["bounded"].sum() > 300
    f = 2.0 ** (5 * power)
    assert np.array_equal(out["site"], base["site"] * f, equal_nan=True)
    assert np.array_equal(out["central"], base["central"] * f, equal_nan=True)


def test_a_257_gon_raises_naming_an_axis_cell():
    import radfoam
    from radfoam_amd import foam

    pts = H._CLOUDS["ring257"]()
    off, adj = foam.delaunay_csr(pts)
    t = _tensors(pts, off, adj)
    with pytest.raises(RuntimeError, match=r"cell_geometry: cell [01] is not supported: a face outgrew 256 vertices"):
        radfoam.cell_moments(*t)
    # with a geometry that had room for the 257-gon (the host build at capacity 512) the operator's own redo kernel says so
    geo = H.cell_geometry(pts, adj, off, cap=512)
    assert geo["bad"] == 0 and geo["bounded"][:2].all()
    roomy = radfoam.CellGeometry(*(torch.from_numpy(np.ascontiguousarray(geo[k])).to(DEV)
                                   for k in ("volume", "centroid", "bounded", "face_area")))
    with pytest.raises(RuntimeError, match=r"cell_moments: cell [01] is not supported: a face outgrew 256 vertices"):
        radfoam.cell_moments(*t, geometry=roomy)


def test_a_malformed_row_raises_naming_the_cell():
    import radfoam

    c = H.case("uniform400")
    t, mo, _ = _device_case("uniform400")
    adj = c["adjacency"].astype(np.int64)
    adj[int(c["offsets"][40])] = 40          # the site itself in its own row
    with pytest.raises(RuntimeError, match=r"cell_moments: cell 40 is not supported: its adjacency row is malformed"):
        radfoam.cell_moments(t[0], torch.from_numpy(adj).to(DEV), t[2], geometry=mo.geometry)


def test_tiny_inputs():
    import radfoam

    tiny = H.tiny_inputs()
    for name, n in (("n1", 1), ("n2", 2), ("n4", 4)):          # every cell is open
        mo = radfoam.cell_moments(*_tensors(*tiny[name]))
        assert mo.site_moment.shape == (n, 6) and mo.central_moment.shape == (n, 6)
        assert bool(torch.isnan(mo.site_moment).all()) and bool(torch.isnan(mo.central_moment).all())
    a = H.EMPTY_ROW_SITE
    full, got = (radfoam.cell_moments(*_tensors(*tiny[k])) for k in ("empty_row_full", "empty_row"))
    assert bool(full.geometry.bounded[a]) and bool(torch.isfinite(full.site_moment[a]).all())
    assert not bool(got.geometry.bounded[a])
    assert bool(torch.isnan(got.site_moment[a]).all()) and bool(torch.isnan(got.central_moment[a]).all())
    rest = np.arange(full.site_moment.shape[0]) != a           # a gather over each cell's own row: the others keep their bits
    for key in ("site_moment", "central_moment"):
        x, y = getattr(got, key).cpu().numpy()[rest], getattr(full, key).cpu().numpy()[rest]
        assert np.array_equal(x, y, equal_nan=True) and np.isfinite(x).any()


def test_geometry_argument_index_dtypes_and_repeat_runs_give_the_same_bits():
    import radfoam

    t, mo, out = _device_case("ring17")
    same = lambda other: (np.array_equal(other.site_moment.cpu().numpy(), out["site"], equal_nan=True)
                          and np.array_equal(other.central_moment.cpu().numpy(), out["central"], equal_nan=True))
    assert np.isfinite(out["site"][:2]).all()
    assert same(radfoam.cell_moments(*t))                                      # two calls
    passed = radfoam.cell_moments(*t, geometry=mo.geometry)                    # geometry= is used as it is
    assert same(passed) and passed.geometry is mo.geometry
    assert same(radfoam.cell_moments(*t, radfoam.cell_geometry(*t)))
    for dtype in (torch.int32, torch.int64):                                   # next to uint32
        assert same(radfoam.cell_moments(t[0], t[1].to(dtype), t[2].to(dtype)))


def test_input_validation():
    import radfoam

    t, mo, _ = _device_case("ring17")
    geo = mo.geometry
    other = _device_case("ring16")[1].geometry
    assert other.volume.shape != geo.volume.shape
    for bad in (other, geo._replace(volume=geo.volume.float()), geo._replace(centroid=geo.centroid.cpu()),
                geo._replace(bounded=geo.bounded.to(torch.uint8)), geo._replace(centroid=geo.centroid[:, :2]), "geo"):
        with pytest.raises(RuntimeError, match="geometry must be the CellGeometry"):
            radfoam.cell_moments(*t, geometry=bad)
    with pytest.raises(RuntimeError, match="points must be a float32 CUDA tensor"):
        radfoam.cell_moments(t[0].double(), t[1], t[2])
    with pytest.raises(RuntimeError, match="must have uint32, int32 or int64 dtype"):
        radfoam.cell_moments(t[0], t[1].to(torch.int64).to(torch.int16), t[2])


def test_the_gpu_triangulation_feeds_straight_in():
    """4,000 uniform points, the GPU's own CSR: on the bounded cells the central moment is positive semidefinite and
    tr site = tr central + V |c - p|^2, both to 1e-9 tr site; unbounded cells are NaN in all twelve."""
    import radfoam
    from radfoam_amd.triangulation import Triangulation

    gen = torch.Generator(device="cpu").manual_seed(0)
    start = (torch.rand((4000, 3), generator=gen) * 2.0 - 1.0).to(DEV)
    tri = Triangulation(start)
    points = start[tri.permutation().to(torch.int64)].contiguous()
    assert tri.point_adjacency().dtype == torch.uint32
    mo = radfoam.cell_moments(points, tri.point_adjacency(), tri.point_adjacency_offsets())
    geo = mo.geometry
    b = geo.bounded
    assert int(b.sum()) > 3000 and int((~b).sum()) > 0
    assert bool(torch.isnan(mo.site_moment[~b]).all()) and bool(torch.isnan(mo.central_moment[~b]).all())
    site, central = mo.site_moment[b], mo.central_moment[b]
    assert bool(torch.isfinite(site).all()) and bool(torch.isfinite(central).all())
    tr_site, tr_central = site[:, :3].sum(1), central[:, :3].sum(1)
    assert bool((tr_site > 0).all())
    shift = geo.volume[b] * ((geo.centroid[b] - points[b].double()) ** 2).sum(1)
    axis = ((tr_site - tr_central - shift).abs() / tr_site).max().item()
    xx, yy, zz, xy, xz, yz = central.unbind(-1)
    sym = torch.stack([torch.stack([xx, xy, xz], -1), torch.stack([xy, yy, yz], -1), torch.stack([xz, yz, zz], -1)], -2)
    low = (torch.linalg.eigvalsh(sym.cpu())[:, 0] / tr_site.cpu()).min().item()
    print(f"triangulation CSR: {int(b.sum())} bounded cells, |tr site - tr central - V |c - p|^2| / tr site = {axis:.3g}, "
          f"smallest eigenvalue of central / tr site = {low:.3g}")
    assert axis <= 1e-9 and low >= -1e-9


def test_the_example_writes_a_ply(tmp_path):
    from examples import foam_to_gaussians as G

    path = tmp_path / "foam.ply"
    written, energy, surrogate = G.run(num_points=2000, out=str(path), device=DEV, quiet=True)
    raw = path.read_bytes()
    head, body = raw.split(b"end_header\n", 1)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\n") and f"element vertex {written}".encode() in head
    table = np.frombuffer(body, dtype="<f4").reshape(written, len(G.PLY_FIELDS))
    assert written > 1500 and np.isfinite(table).all()
    assert np.abs(np.linalg.norm(table[:, 13:17], axis=1) - 1.0).max() <= 1e-6
    assert 0.0 < surrogate < energy
