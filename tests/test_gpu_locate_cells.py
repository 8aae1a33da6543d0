"""radfoam.locate_cells on the device: the kernel of csrc/rf_nearest.hip against the host build of the same header
(tests/host_harness/nearest_host.cpp), the faults, Triangulation.locate_cells and locate(nearest="walk"), the untouched
default of locate, and the fp32 brute-force operator."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import locate_ref
from tests import nearest_ref as R
from tests.host_harness import locate_host
from tests.host_harness import nearest_host as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CLOUDS = [("uniform", 400), ("clustered", 400), ("hub", 301)]


def _d(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _list(x, dtype):
    t = _d(np.asarray(x).astype(np.int64))
    if dtype == "misaligned":                                          # int32 words 4 bytes off a 16-byte boundary
        buf = torch.empty(t.numel() + 1, dtype=torch.int32, device=DEV)
        buf[1:] = t.to(torch.int32)
        view = buf[1:]
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view
    return t.to(torch.int32).view(torch.uint32) if dtype == torch.uint32 else t.to(dtype)


def _locate(points, adj, offsets, q, dtype=torch.uint32, **kw):
    import radfoam
    if kw.get("start") is not None:
        kw["start"] = _d(np.asarray(kw["start"]).astype(np.int64))
    got = radfoam.locate_cells(_d(points), _list(adj, dtype), _list(offsets, torch.uint32 if dtype == "misaligned" else dtype),
                               _d(q), **kw)
    assert got.cell.is_cuda and got.cell.dtype == torch.int64 and got.hops.dtype == torch.int32
    return got.cell.cpu().numpy(), got.hops.cpu().numpy()


@pytest.mark.parametrize("kind,n", CLOUDS)
def test_the_kernel_equals_the_host_build(kind, n):
    m, q = R.cloud(kind, n), R.queries(kind, n)["q"]
    for kw in ({}, dict(seeds=0), dict(start=R.given_starts(kind, n))):
        host = H.locate(m["points"], m["adjacency"], m["offsets"], q, **kw)
        for dtype in (torch.uint32, torch.uint32, torch.int32, torch.int64, "misaligned"):   # and a second run
            cell, hops = _locate(m["points"], m["adjacency"], m["offsets"], q, dtype, **kw)
            assert np.array_equal(cell, host["cell"]) and np.array_equal(hops, host["hops"]), (kw.keys(), dtype)
        assert R.check_nearest(kind, n, host["cell"]) == 0


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 257])
def test_query_counts_and_shapes(count):
    import radfoam
    m, q = R.cloud("uniform", 400), R.queries("uniform", 400)["q"][:count]
    host = H.locate(m["points"], m["adjacency"], m["offsets"], q)
    cell, hops = _locate(m["points"], m["adjacency"], m["offsets"], q)
    assert cell.shape == (count,) and np.array_equal(cell, host["cell"]) and np.array_equal(hops, host["hops"])
    if count == 257:
        grid = radfoam.locate_cells(_d(m["points"]), _list(m["adjacency"], torch.uint32), _list(m["offsets"], torch.uint32),
                                    _d(q[:256]).reshape(16, 16, 3))
        assert grid.cell.shape == (16, 16) and grid.hops.shape == (16, 16)
        assert np.array_equal(grid.cell.cpu().numpy().reshape(-1), host["cell"][:256])
        assert np.array_equal(grid.hops.cpu().numpy().reshape(-1), host["hops"][:256])


@pytest.mark.parametrize("n", [64, 400, 3000])
@pytest.mark.parametrize("seeds", [1, 7, 1024])
def test_site_counts_and_seeds(n, seeds):
    m, q = R.cloud("uniform", n), R.queries("uniform", n)["q"]
    host = H.locate(m["points"], m["adjacency"], m["offsets"], q, seeds=seeds)
    cell, hops = _locate(m["points"], m["adjacency"], m["offsets"], q, seeds=seeds)
    assert np.array_equal(cell, host["cell"]) and np.array_equal(hops, host["hops"])
    assert R.check_nearest("uniform", n, cell) == 0
    if n == 64 and seeds == 1024:
        assert (hops == 0).all()                                       # every site is a seed


def test_faults_raise_as_on_the_host_and_leave_nothing_behind():
    m = R.cloud("uniform", 400)
    valid = R.valid_queries(m)
    want = H.locate(m["points"], m["adjacency"], m["offsets"], valid)
    for name, (adj, off, start, q) in R.malformed(m).items():
        host = H.locate(m["points"], adj, off, q, start=start)
        first = int(np.nonzero(host["cell"] < -1)[0][0])
        for dtype in (torch.int64, torch.int32):
            with pytest.raises(RuntimeError, match=f"locate_cells: query {first}:"):
                _locate(m["points"], adj, off, q, dtype, start=start)
            cell, hops = _locate(m["points"], m["adjacency"], m["offsets"], valid)
            assert np.array_equal(cell, want["cell"]) and np.array_equal(hops, want["hops"]), name


def test_the_capped_walk_raises_and_does_not_hang():
    m, q = R.cloud("uniform", 400), R.queries("uniform", 400)["q"]
    host = H.locate(m["points"], m["adjacency"], m["offsets"], q, seeds=0, max_hops=2)
    first = int(np.nonzero(host["cell"] < -1)[0][0])
    with pytest.raises(RuntimeError, match=f"query {first}: its walk would take more than max_hops = 2"):
        _locate(m["points"], m["adjacency"], m["offsets"], q, seeds=0, max_hops=2)
    whole = H.locate(m["points"], m["adjacency"], m["offsets"], q, seeds=0)
    cell, hops = _locate(m["points"], m["adjacency"], m["offsets"], q, seeds=0)
    assert np.array_equal(cell, whole["cell"]) and np.array_equal(hops, whole["hops"])


def _tree_start(tri, q):
    """what Triangulation.locate starts its walks at by default, computed here"""
    from radfoam_amd.scene_ops import nearest_point_tree
    from radfoam_amd.triangulation import build_aabb_tree
    finite = torch.isfinite(q).all(-1, keepdim=True)
    site = nearest_point_tree(tri._points, build_aabb_tree(tri._points), torch.where(finite, q, torch.zeros_like(q)))
    return tri.vert_to_tet().view(torch.int32)[site.view(torch.int32).to(torch.int64).clamp(0, tri._points.size(0) - 1)]


def test_triangulation_locate_cells_the_walk_start_and_an_incremental_rebuild():
    import radfoam
    from tests import tets_ref
    pts = torch.from_numpy(tets_ref.uniform(5001, seed=31)).to(DEV)
    tri = radfoam.Triangulation(pts)
    rng = np.random.default_rng(32)
    q = np.concatenate([rng.uniform(-1.1, 1.1, (400, 3)), [[np.nan, 0, 0], [0, np.inf, 0]]]).astype(np.float32)

    def check():
        p, adj, off = tri._points.cpu().numpy(), tri.point_adjacency().cpu().numpy(), tri.point_adjacency_offsets().cpu().numpy()
        got = tri.locate_cells(_d(q))
        host = H.locate(p, adj, off, q)
        assert np.array_equal(got.cell.cpu().numpy(), host["cell"]) and np.array_equal(got.hops.cpu().numpy(), host["hops"])
        for k in range(0, 400, 8):
            assert int(host["cell"][k]) in R.nearest_sites(p, q[k]).tolist(), k
        # the default of locate: bit for bit locate_tets from the tree's starts
        default = tri.locate(_d(q))
        own = radfoam.locate_tets(tri._points, tri.tets(), tri.tet_adjacency(), _d(q), start=_tree_start(tri, _d(q)))
        assert torch.equal(default.tet, own.tet) and torch.equal(default.hops, own.hops)
        # nearest="walk": every query located exactly, the same tetrahedron wherever the query is strictly interior
        tree = tri._tree
        tri._tree = None
        walked = tri.locate(_d(q), nearest="walk")
        assert tri._tree is None                                       # the walk builds no tree
        tri._tree = tree
        tet, mesh = walked.tet.cpu().numpy(), dict(points=p, tets=tri.tets().cpu().numpy().astype(np.int64))
        locate_ref.check_located(mesh, q, tet)
        theirs = default.tet.cpu().numpy()
        for k in np.nonzero(tet != theirs)[0]:
            assert not locate_ref.strictly_inside(p, mesh["tets"][theirs[k]], q[k]), k
        start = tri.vert_to_tet().view(torch.int32)[got.cell.clamp(0, 5000)]
        again = locate_host.walk(p, mesh["tets"], tri.tet_adjacency().cpu().numpy(), q, start.cpu().numpy())
        assert np.array_equal(tet, again["tet"]) and np.array_equal(walked.hops.cpu().numpy(), again["hops"])
        return got

    first = check()
    gen = torch.Generator().manual_seed(33)
    moved = (tri._points.cpu() + 0.02 * torch.randn((5001, 3), generator=gen)).to(DEV)
    assert tri.rebuild(moved, incremental=True) is False
    second = check()
    assert not torch.equal(first.cell, second.cell)


def test_uniform_queries_against_the_fp32_operator():
    """Equal to nearest_point except where the two candidates' fp32 squared distances are within rounding of each other (at
    most 5 roundings of 2^-24 each way, 12 with the second order: tests/test_locate_cells.py), and there the exact
    predicate sides with locate_cells."""
    from radfoam_amd.nearest import exact_closer
    from radfoam_amd.scene_ops import nearest_point
    m = R.cloud("uniform", 3000)
    q = np.random.default_rng(41).uniform(-1.1, 1.1, (2000, 3)).astype(np.float32)
    cell, _ = _locate(m["points"], m["adjacency"], m["offsets"], q)
    theirs = nearest_point(_d(m["points"]), _d(q)).view(torch.int32).cpu().numpy().astype(np.int64)
    differ = np.nonzero(cell != theirs)[0]
    print(f"{len(differ)} of {len(q)} uniform queries differ from nearest_point (fp32 keys within rounding)")
    for k in differ:
        d = m["points"][[cell[k], theirs[k]]] - q[k]
        mine, other = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float64)
        assert abs(mine - other) <= 12 * 2.0 ** -24 * max(mine, other), k
        assert exact_closer(m["points"][cell[k]], m["points"][theirs[k]], q[k]) <= 0, k
