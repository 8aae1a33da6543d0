"""Voronoi cell geometry on the GPU (radfoam.cell_geometry / cell_surface) against Qhull: scipy.spatial.Voronoi +
ConvexHull per region, in double.  The cloud is N = 1500 fp32 points uniform in [-1,1]^3 (seed 2) with Qhull's
adjacency, h = (bbox volume / N)^(1/3); a second cloud holds a 48-gon face.

The bars (tests/host_harness/clip_host.check_cells / check_faces) are 1e-9 h^3 / h^2 / h: the clipping core in double
differs from Qhull by ~1e-13 h^3 (tests/test_cell_geometry.py measures it on the host), in float32 by ~2e-6 h^3, and a
missed clip plane is O(h^3)."""
import numpy as np
import pytest
import torch

from tests.host_harness import clip_host as H

pytestmark = pytest.mark.gpu

_GPU = {}


def _device_case(name):
    """The case's tensors on the device and cell_geometry's answer for them (computed once, as numpy)."""
    if name not in _GPU:
        import radfoam

        c = H.case(name)
        dev = "cuda:0"
        t = dict(points=torch.from_numpy(c["points"]).to(dev),
                 adjacency=torch.from_numpy(c["adjacency"].astype(np.int64)).to(dev).to(torch.uint32),
                 offsets=torch.from_numpy(c["offsets"].astype(np.int64)).to(dev).to(torch.uint32))
        geo = radfoam.cell_geometry(t["points"], t["adjacency"], t["offsets"])
        assert isinstance(geo, radfoam.CellGeometry)
        assert geo.volume.dtype == torch.float64 and geo.volume.shape == (len(c["points"]),)
        assert geo.centroid.dtype == torch.float64 and geo.centroid.shape == (len(c["points"]), 3)
        assert geo.bounded.dtype == torch.bool and geo.face_area.shape == (len(c["adjacency"]),)
        t["geo"] = geo
        t["np"] = {k: getattr(geo, k).cpu().numpy() for k in geo._fields}
        _GPU[name] = t
    return _GPU[name]


def test_volumes_centroids_and_flags_match_qhull():
    c, t = H.case("uniform"), _device_case("uniform")
    assert c["ref"]["compared"].sum() >= 0.8 * len(c["points"])
    H.check_cells(c, t["np"]["volume"], t["np"]["centroid"], t["np"]["bounded"])


def test_face_identities():
    c, t = H.case("uniform"), _device_case("uniform")
    H.check_faces(c, t["np"]["volume"], t["np"]["bounded"], t["np"]["face_area"])


def test_a_48_gon_face():
    c, t = H.case("ring"), _device_case("ring")
    assert c["ref"]["ridge_vertices"][(0, 1)] == 48 and c["ref"]["compared"][:2].all()
    H.check_cells(c, t["np"]["volume"], t["np"]["centroid"], t["np"]["bounded"])
    H.check_faces(c, t["np"]["volume"], t["np"]["bounded"], t["np"]["face_area"])


def test_index_dtypes_agree():
    import radfoam

    t = _device_case("uniform")
    for dtype in (torch.int32, torch.int64):
        geo = radfoam.cell_geometry(t["points"], t["adjacency"].to(dtype), t["offsets"].to(dtype))
        assert torch.equal(geo.bounded, t["geo"].bounded)
        assert np.array_equal(geo.volume.cpu().numpy(), t["np"]["volume"], equal_nan=True)
        assert np.array_equal(geo.face_area.cpu().numpy(), t["np"]["face_area"], equal_nan=True)


def test_a_malformed_row_raises_naming_the_cell():
    import radfoam

    c, t = H.case("uniform"), _device_case("uniform")
    adj = c["adjacency"].astype(np.int64)
    adj[int(c["offsets"][40])] = 40          # the site itself in its own row
    with pytest.raises(RuntimeError, match="cell 40 "):
        radfoam.cell_geometry(t["points"], torch.from_numpy(adj).to("cuda:0"), t["offsets"])


def test_surface_of_a_ball_of_cells():
    import radfoam

    c, t = H.case("uniform"), _device_case("uniform")
    pts, h = c["points"].astype(np.float64), c["h"]
    rows, adj = c["rows"], c["adjacency"].astype(np.int64)
    inside = np.linalg.norm(pts, axis=1) < 0.5
    assert inside.sum() > 50 and t["np"]["bounded"][inside].all()
    tri, edge = radfoam.cell_surface(t["points"], t["adjacency"], t["offsets"], torch.from_numpy(inside).to("cuda:0"))
    assert tri.dtype == torch.float64 and edge.dtype == torch.int64 and tri.shape == (edge.numel(), 3, 3)
    tri, edge = tri.cpu().numpy(), edge.cpu().numpy()
    straddle = inside[rows] & ~inside[adj]
    # every triangle comes from a straddling slot, in slot order; T = sum (face vertices - 2), Qhull's vertex counts
    assert straddle[edge].all() and (np.diff(edge) >= 0).all()
    want = np.array([c["ref"]["ridge_vertices"][(int(a), int(b))] - 2 for a, b in zip(rows[straddle], adj[straddle])])
    assert np.array_equal(np.bincount(edge, minlength=len(adj))[straddle], want) and len(edge) == want.sum()
    # closed: the enclosed volume is the cells' volume
    enclosed = np.einsum("ij,ij->i", tri[:, 0], np.cross(tri[:, 1], tri[:, 2])).sum() / 6.0
    total = t["np"]["volume"][inside].sum()
    print(f"surface: {len(edge)} triangles, enclosed - sum V = {(enclosed - total) / h ** 3:.3g} h^3")
    assert abs(enclosed - total) <= 1e-9 * h ** 3 * inside.sum()
    # the triangles of a face tile it, and face outwards (a -> b)
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    area = 0.5 * np.linalg.norm(normal, axis=1).sum()
    faces = t["np"]["face_area"][straddle].sum()
    print(f"surface: area - sum face_area = {(area - faces) / h ** 2:.3g} h^2")
    assert abs(area - faces) <= 1e-9 * h ** 2 * straddle.sum()
    assert (np.einsum("ij,ij->i", normal, pts[adj[edge]] - pts[rows[edge]]) > 0).all()
    # a hull cell cannot be selected
    hull = int(np.nonzero(c["ref"]["unbounded"])[0][0])
    mask = torch.zeros(len(pts), dtype=torch.bool, device="cuda:0")
    mask[hull] = True
    with pytest.raises(ValueError, match="unbounded"):
        radfoam.cell_surface(t["points"], t["adjacency"], t["offsets"], mask)


def test_surface_through_the_48_gon():
    import radfoam

    c, t = H.case("ring"), _device_case("ring")
    inside = torch.zeros(len(c["points"]), dtype=torch.bool, device="cuda:0")
    inside[0] = True
    tri, edge = radfoam.cell_surface(t["points"], t["adjacency"], t["offsets"], inside)
    tri, edge = tri.cpu().numpy(), edge.cpu().numpy()
    slot = int(c["offsets"][0]) + int(np.searchsorted(c["adjacency"][c["offsets"][0]:c["offsets"][1]], 1))
    assert (edge == slot).sum() == 46
    enclosed = np.einsum("ij,ij->i", tri[:, 0], np.cross(tri[:, 1], tri[:, 2])).sum() / 6.0
    assert abs(enclosed - t["np"]["volume"][0]) <= 1e-9 * c["h"] ** 3


def test_the_gpu_triangulation_feeds_straight_in():
    import radfoam
    from radfoam_amd.triangulation import Triangulation

    c, t = H.case("uniform"), _device_case("uniform")
    tri = Triangulation(t["points"])
    perm = tri.permutation().to(torch.int64)
    assert tri.point_adjacency().dtype == torch.uint32
    geo = radfoam.cell_geometry(t["points"][perm], tri.point_adjacency(), tri.point_adjacency_offsets())
    volume = np.empty(len(perm))
    bounded = np.empty(len(perm), dtype=bool)
    volume[perm.cpu().numpy()] = geo.volume.cpu().numpy()
    bounded[perm.cpu().numpy()] = geo.bounded.cpu().numpy()
    was = t["np"]["bounded"]
    assert bounded[was].all()
    diff = np.abs(volume[was] - t["np"]["volume"][was]).max()
    print(f"triangulation CSR: max |dV| = {diff / c['h'] ** 3:.3g} h^3")
    assert diff <= 1e-9 * c["h"] ** 3


# ---- the kernel's seams, against the exact reference (tests/cell_geometry_ref.py) ----------------------------------------
#
# Bars are per cell, in units of its own size s_a = V_ref,a^(1/3): 1e-9 s_a^3 / s_a^2 / s_a (clip_host.check_cells /
# check_faces with local=True).  The CPU twins in tests/test_cell_geometry.py assert the construction of every cloud.
# Worst ratios measured on the MI355X (|dV| / s^3, |dc| / s, |dA| / s^2; the host build gives the same figures):
#   ring16 3e-15 2e-15 1e-14, ring17 1e-14 4e-15 1e-14, ring256 9e-14 2e-13 2e-13, hub64/65 1e-14 4e-15 5e-14,
#   hub200 2e-14 9e-15 1e-13, redo_spread 1.2e-14 8.7e-15 8.0e-14, uniform400 and both scalings 1.2e-14 4.9e-15 4.4e-14,
#   offset 8.4e-15 2.0e-13 2.9e-14, grid 1.6e-15 6.7e-16 7e-15,
#   clustered 1.2e-10 4.4e-11 2.9e-10 (symmetry 4.2e-10, closure 4.3e-10): R = 4 |diagonal| is about 1e6 of its smallest
#   cells and the first clips of the square cost that much; still under 1e-9, so the bar was not widened and no Qhull
#   yardstick was needed.  Either-way share: 0 % on the ring, hub, redo and grid clouds, 3.1 % on the 400-site clouds,
#   1.4 % on clustered.  Both scalings equal the unscaled cloud times 2^+-30 / 2^+-20 / 2^+-10 bit for bit.

def _device_tensors(points, offsets, adjacency):
    dev = "cuda:0"
    return (torch.from_numpy(points).to(dev), torch.from_numpy(adjacency.astype(np.int64)).to(dev).to(torch.uint32),
            torch.from_numpy(offsets.astype(np.int64)).to(dev).to(torch.uint32))


def _device_out(name):
    """cell_geometry's answer plus face_vertices (the count cell_surface works from), as numpy"""
    from radfoam_amd import geometry

    t = _device_case(name)
    if "out" not in t:
        _, nv = geometry._run_geometry(*geometry._prepare(t["points"], t["adjacency"], t["offsets"]))
        t["out"] = dict(t["np"], face_vertices=nv.cpu().numpy())
    return t["out"]


def _surface(name, inside):
    import radfoam

    t = _device_case(name)
    tri, edge = radfoam.cell_surface(t["points"], t["adjacency"], t["offsets"], torch.from_numpy(inside).to("cuda:0"))
    assert tri.dtype == torch.float64 and edge.dtype == torch.int64
    return tri.cpu().numpy(), edge.cpu().numpy()


@pytest.mark.parametrize("k", [16, 17, 256])
def test_a_k_gon_at_the_capacity_of_the_lane_path_and_of_the_serial_path(k):
    """16 vertices stay in the lane's LDS slot, 17 hand both axis cells on (and leave every other cell as it was), 256
    fill the serial path."""
    c, out = H.case(f"ring{k}"), _device_out(f"ring{k}")
    assert out["face_vertices"][H.slot_of(c, 0, 1)] == k == out["face_vertices"][H.slot_of(c, 1, 0)]
    H.check_against_exact(c, out, cells=np.array([0, 1]))
    H.check_against_exact(c, out)


def test_a_257_gon_raises_naming_an_axis_cell():
    import radfoam
    from radfoam_amd import foam

    pts = H._CLOUDS["ring257"]()
    off, adj = foam.delaunay_csr(pts)
    with pytest.raises(RuntimeError, match=r"cell [01] is not supported: a face outgrew 256 vertices"):
        radfoam.cell_geometry(*[_device_tensors(pts, off, adj)[i] for i in (0, 1, 2)])


@pytest.mark.parametrize("k", [64, 65, 200])
def test_a_row_of_64_faces_on_the_wave_path_and_longer_rows_on_the_serial_path(k):
    c, out = H.case(f"hub{k}"), _device_out(f"hub{k}")
    assert int(c["offsets"][1]) == k
    assert np.isfinite(out["face_area"][:k]).all() and (out["face_area"][:k] > 0).all()
    assert np.array_equal(out["face_vertices"][:k].astype(np.int64), c["slots"]["vertices"][:k])
    H.check_against_exact(c, out, cells=np.arange(k + 1))
    H.check_against_exact(c, out)


def test_handed_on_cells_in_several_blocks_of_the_redo_kernel():
    c, out = H.case("redo_spread"), _device_out("redo_spread")
    pairs = np.array(H.REDO_SPREAD_PAIRS)
    for a, b in pairs:
        assert out["face_vertices"][H.slot_of(c, int(a), int(b))] == 17
    H.check_against_exact(c, out, cells=pairs.reshape(-1))
    in_blocks = np.isin(np.arange(len(c["points"])) // 64, pairs[:, 0] // 64) & ~c["exact"]["open"]
    H.check_against_exact(c, out, cells=np.nonzero(in_blocks)[0])


@pytest.mark.parametrize("name", ["clustered", "uniform400", "offset", "scaled_small", "scaled_large"])
def test_cells_of_very_different_sizes_far_from_the_origin_and_scaled(name):
    c, out = H.case(name), _device_out(name)
    H.check_against_exact(c, out, share=None if name == "clustered" else 0.05)
    if name.startswith("scaled"):       # a power of two commutes with every operation of rf_clip.hpp: bit for bit
        f = 2.0 ** (-10 if name == "scaled_small" else 10)
        base = _device_out("uniform400")
        assert np.array_equal(out["volume"], base["volume"] * f ** 3)
        assert np.array_equal(out["centroid"], base["centroid"] * f, equal_nan=True)
        assert np.array_equal(out["face_area"], base["face_area"] * f ** 2)


def test_a_grid_of_cospherical_sites():
    c, out = H.case("grid"), _device_out("grid")
    H.check_grid(c, out)
    H.check_against_exact(c, out, vertices=False)


def test_tiny_inputs():
    import radfoam

    tiny = H.tiny_inputs()
    run = lambda name: radfoam.cell_geometry(*_device_tensors(*tiny[name]))
    geo = run("n4")
    assert not geo.bounded.any() and torch.isposinf(geo.volume).all() and torch.isnan(geo.centroid).all()
    assert torch.isposinf(geo.face_area).all()
    for name, n in (("n1", 1), ("n2", 2)):
        geo = run(name)
        assert geo.volume.shape == (n,) and geo.face_area.shape == (0,)
        assert not geo.bounded.any() and torch.isposinf(geo.volume).all() and torch.isnan(geo.centroid).all()
    a = H.EMPTY_ROW_SITE
    full, got = run("empty_row_full"), run("empty_row")
    assert bool(full.bounded[a]) and not bool(got.bounded[a])
    assert torch.isposinf(got.volume[a]) and torch.isnan(got.centroid[a]).all()
    rest = np.arange(full.volume.numel()) != a
    for key in ("volume", "centroid", "bounded"):
        assert np.array_equal(getattr(got, key).cpu().numpy()[rest], getattr(full, key).cpu().numpy()[rest],
                              equal_nan=True)


def test_surface_of_the_hub_of_200_faces():
    c = H.case("hub200")
    inside = np.zeros(len(c["points"]), dtype=bool)
    inside[0] = True
    tri, edge = _surface("hub200", inside)
    assert len(edge) == (c["slots"]["vertices"][:200] - 2).sum()
    H.check_surface(c, inside, tri, edge, c["exact"]["volume_f"][0], np.cbrt(c["exact"]["volume_f"][0]))


def test_surface_of_a_block_of_grid_cells():
    c = H.case("grid")
    block = np.zeros((6, 6, 6), dtype=bool)
    block[2:4, 2:4, 2:4] = True
    tri, edge = _surface("grid", block.reshape(-1))
    H.check_surface(c, block.reshape(-1), tri, edge, 8 * H.GRID_H ** 3, H.GRID_H, area=24 * H.GRID_H ** 2,
                    counts=False)      # zero-area faces of cospherical sites have whatever count they have


def test_surface_of_an_axis_cell_of_the_17_gon():
    c = H.case("ring17")
    inside = np.zeros(len(c["points"]), dtype=bool)
    inside[1] = True
    tri, edge = _surface("ring17", inside)
    assert (edge == H.slot_of(c, 1, 0)).sum() == 15
    H.check_surface(c, inside, tri, edge, c["exact"]["volume_f"][1], np.cbrt(c["exact"]["volume_f"][1]))
