"""radfoam.delaunay_tets on the device: the kernels of csrc/rf_tets.hip against the host build of the same header
(tests/host_harness/tets_host.cpp) and Qhull's canonicalised rows (tests/tets_ref.py), the GPU Triangulation's getters,
isosurface on their rows, and the errors."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from radfoam_amd.triangulation import TriangulationFailedError
from tests import tets_ref as R
from tests.host_harness import iso_host as HI
from tests.host_harness import tets_host as HT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_HOST = {}


def _host(kind, n):
    if (kind, n) not in _HOST:
        ref = R.cloud(kind, n)
        _HOST[(kind, n)] = HT.delaunay_tets(ref["points"], ref["adjacency"], ref["offsets"])
    return _HOST[(kind, n)]


def _run(points, adj, off, dtype=torch.uint32, adjacency=True):
    import radfoam
    def as_t(x):
        t = torch.from_numpy(np.asarray(x).astype(np.int64)).to(DEV)
        return t.to(torch.int32).view(torch.uint32) if dtype == torch.uint32 else t.to(dtype)
    return radfoam.delaunay_tets(torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).to(DEV), as_t(adj),
                                 as_t(off), adjacency=adjacency)


def _same(got, host):
    assert got.tets.is_cuda and got.tets.dtype == torch.uint32 and got.vert_to_tet.dtype == torch.uint32
    assert np.array_equal(got.tets.cpu().numpy(), host["tets"])
    assert np.array_equal(got.vert_to_tet.cpu().numpy(), host["vert_to_tet"])
    assert np.array_equal(got.tet_adjacency.cpu().numpy(), host["tet_adjacency"])
    assert got.hull_faces == host["hull_faces"]


@pytest.mark.parametrize("kind,n", R.CLOUDS + [("hub", 100), ("hub", 300)])
def test_kernels_equal_the_host_build(kind, n):
    ref, host = R.cloud(kind, n), _host(kind, n)
    if kind == "hub":
        assert host["code"][0] == (4 if n == 100 else 5)           # the second and the third star instance
    first = _run(ref["points"], ref["adjacency"], ref["offsets"])
    _same(first, host)
    R.check_against(ref, first.tets.cpu().numpy(), first.vert_to_tet.cpu().numpy(), first.tet_adjacency.cpu().numpy(),
                    first.hull_faces)
    for dtype in (torch.uint32, torch.int32, torch.int64):          # a second run, and every list dtype
        _same(_run(ref["points"], ref["adjacency"], ref["offsets"], dtype), host)
    assert _run(ref["points"], ref["adjacency"], ref["offsets"], adjacency=False).tet_adjacency is None


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_wave_seams_every_site_emits_its_owned_rows(n):
    ref = R.reference(R.uniform(n, seed=10 + n))
    got = _run(ref["points"], ref["adjacency"], ref["offsets"])
    tets = got.tets.cpu().numpy().astype(np.int64)
    assert np.array_equal(tets, ref["tets"])
    assert np.array_equal(np.bincount(tets[:, 0], minlength=n), np.bincount(ref["tets"][:, 0], minlength=n))
    assert np.array_equal(R._signed(got.vert_to_tet.cpu().numpy()), ref["vert_to_tet"])


def test_adjacency_from_tets_gives_the_lists_back():
    from radfoam_amd import scene_ops
    ref = R.cloud("uniform", 3000)
    got = _run(ref["points"], ref["adjacency"], ref["offsets"], adjacency=False)
    adj, off = scene_ops.adjacency_from_tets(got.tets, 3000)
    assert np.array_equal(adj.cpu().numpy(), ref["adjacency"]) and np.array_equal(off.cpu().numpy(), ref["offsets"])


def test_triangulation_getters_run_the_operator_and_follow_a_rebuild():
    import radfoam
    pts = torch.from_numpy(R.uniform(5001, seed=21)).to(DEV)
    tri = radfoam.Triangulation(pts)
    ordered = pts[tri.permutation().to(torch.int64)]
    ref = R.reference(ordered.cpu().numpy())
    assert np.array_equal(tri.point_adjacency().cpu().numpy(), ref["adjacency"])
    own = radfoam.delaunay_tets(ordered, tri.point_adjacency(), tri.point_adjacency_offsets(), adjacency=True)
    assert torch.equal(tri.tets(), own.tets) and torch.equal(tri.vert_to_tet(), own.vert_to_tet)
    assert torch.equal(tri.tet_adjacency(), own.tet_adjacency)
    assert tri.tets() is tri.tets()                                  # kept, not computed again
    R.check_against(ref, tri.tets().cpu().numpy(), tri.vert_to_tet().cpu().numpy(), tri.tet_adjacency().cpu().numpy(),
                    own.hull_faces)
    before = tri.tets().clone()
    gen = torch.Generator().manual_seed(3)
    moved = (ordered.cpu() + 0.02 * torch.randn((5001, 3), generator=gen)).to(DEV)
    assert tri.rebuild(moved, incremental=True) is False
    host = HT.delaunay_tets(moved.cpu().numpy(), tri.point_adjacency().cpu().numpy(),
                            tri.point_adjacency_offsets().cpu().numpy())
    after = tri.tets()
    assert np.array_equal(after.cpu().numpy(), host["tets"])
    assert after.shape != before.shape or not torch.equal(after, before)   # the new mesh, not the kept one
    assert np.array_equal(tri.vert_to_tet().cpu().numpy(), host["vert_to_tet"])
    assert np.array_equal(tri.tet_adjacency().cpu().numpy(), host["tet_adjacency"])


def _np_mesh(m):
    return dict(vertices=m.vertices.detach().cpu().numpy(), vertex_sites=m.vertex_sites.cpu().numpy(),
                triangles=m.triangles.cpu().numpy(), triangle_tet=m.triangle_tet.cpu().numpy())


def test_isosurface_on_the_getters_rows():
    import radfoam
    from scipy.spatial import Delaunay
    pts = torch.from_numpy(R.uniform(2000, seed=22)).to(DEV)
    tri = radfoam.Triangulation(pts)
    p = pts[tri.permutation().to(torch.int64)].contiguous()
    values = (0.6 - p.to(torch.float64).norm(dim=1)).to(torch.float32)
    tets = tri.tets()
    mine = _np_mesh(radfoam.isosurface(p, tets, values, 0.0))
    HI.check_closed(mine, "isosurface on Triangulation.tets()")       # closed, oriented, V - E + F = 2
    qhull = torch.from_numpy(Delaunay(p.cpu().numpy().astype(np.float64)).simplices.astype(np.int64)).to(DEV)
    theirs = _np_mesh(radfoam.isosurface(p, qhull, values, 0.0))
    as_set = lambda m: {tuple(s) for s in m["vertex_sites"].tolist()}
    assert as_set(mine) == as_set(theirs)
    # the area vectors tetrahedron by tetrahedron (rows matched by their site sets) and summed
    a, b = HI.area_vectors(mine, len(tets)), HI.area_vectors(theirs, len(qhull))
    key = lambda rows: np.sort(rows.cpu().numpy().astype(np.int64), axis=1)
    ka, kb = key(tets), key(qhull)
    assert np.array_equal(ka[np.lexsort(ka.T[::-1])], kb[np.lexsort(kb.T[::-1])])
    a, b = a[np.lexsort(ka.T[::-1])], b[np.lexsort(kb.T[::-1])]
    scale = np.abs(b).max()
    worst, total = np.abs(a - b).max() / scale, np.abs(a.sum(0) - b.sum(0)).max() / scale
    print(f"area vectors: per tetrahedron {worst:.3g}, summed {total:.3g} of the largest")
    assert worst <= 1e-12 and total <= 1e-12


def test_errors_raise_and_leave_nothing_behind():
    ref, host = R.cloud("uniform", 400), _host("uniform", 400)
    for name, (adj, off) in R.malformed_lists(ref).items():
        with pytest.raises(RuntimeError) as err:
            _run(ref["points"], adj, off, torch.int64)
        assert not isinstance(err.value, TriangulationFailedError), name
        _same(_run(ref["points"], ref["adjacency"], ref["offsets"]), host)
    for name, (adj, off) in R.stale_lists(ref).items():
        with pytest.raises(TriangulationFailedError):
            _run(ref["points"], adj, off, torch.int64)
        _same(_run(ref["points"], ref["adjacency"], ref["offsets"]), host)


def test_lattice_raises_or_returns_a_checked_mesh():
    def run(pts, adj, off):
        got = _run(pts, adj, off)
        return got.tets.cpu().numpy(), got.vert_to_tet.cpu().numpy(), got.tet_adjacency.cpu().numpy(), got.hull_faces
    host = lambda pts, adj, off: (lambda g: (g["tets"], g["vert_to_tet"], g["tet_adjacency"], g["hull_faces"]))(
        HT.delaunay_tets(pts, adj, off))
    assert R.lattice_outcome(run) == R.lattice_outcome(host)
