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
