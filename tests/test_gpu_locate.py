"""radfoam.locate_tets / interpolate / interpolate_grad on the device: the kernels of csrc/rf_locate.hip against the host
build of the same header (tests/host_harness/locate_host.cpp), Triangulation.locate, the errors, and the isosurface's
vertices interpolated back to their level."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import locate_ref as R
from tests.host_harness import locate_host as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MESHES = [("uniform", 400), ("clustered", 400)]


def _d(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _table(x, dtype):
    t = _d(np.asarray(x).astype(np.int64))
    if dtype == "misaligned":                                          # int32 words 8 bytes off a 16-byte boundary
        buf = torch.empty(t.numel() + 2, dtype=torch.int32, device=DEV)
        buf[2:] = t.to(torch.int32).reshape(-1)
        view = buf[2:].view(-1, 4)
        assert view.data_ptr() % 16 == 8 and view.is_contiguous()
        return view
    return t.to(torch.int32).view(torch.uint32) if dtype == torch.uint32 else t.to(dtype)


def _locate(m, q, start=None, dtype=torch.uint32, max_hops=None, tets=None, adjacency=None):
    import radfoam
    got = radfoam.locate_tets(_d(m["points"]), _table(m["tets"] if tets is None else tets, dtype),
                              _table(m["tet_adjacency"] if adjacency is None else adjacency, dtype), _d(q),
                              start=None if start is None else _d(start), max_hops=max_hops)
    assert got.tet.is_cuda and got.tet.dtype == torch.int64 and got.hops.dtype == torch.int32
    return got.tet.cpu().numpy(), got.hops.cpu().numpy()


@pytest.mark.parametrize("kind,n", MESHES)
def test_walk_equals_the_host_build(kind, n):
    m, q = R.mesh(kind, n), R.queries(kind, n)["q"]
    for start in (None, R.nearest_start(m, q)):
        host = H.walk(m["points"], m["tets"], m["tet_adjacency"], q, start)
        for dtype in (torch.uint32, torch.uint32, torch.int32, torch.int64, "misaligned"):   # and a second run
            tet, hops = _locate(m, q, start, dtype)
            assert np.array_equal(tet, host["tet"]) and np.array_equal(hops, host["hops"]), dtype
    R.check_located(m, q, host["tet"])


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 257])
def test_query_counts_and_shapes(count):
    import radfoam
    m, q = R.mesh("uniform", 400), R.queries("uniform", 400)["q"][:count]
    host = H.walk(m["points"], m["tets"], m["tet_adjacency"], q)
    tet, hops = _locate(m, q)
    assert tet.shape == (count,) and np.array_equal(tet, host["tet"]) and np.array_equal(hops, host["hops"])
    values = np.random.default_rng(count).normal(size=400).astype(np.float32)
    got = radfoam.interpolate(_d(m["points"]), _table(m["tets"], torch.uint32), _d(values), _d(q), _d(tet))
    want = H.interpolate(m["points"], m["tets"], values, q, tet)
    assert got.value.shape == (count,) and np.array_equal(got.value.cpu().numpy(), want["value"][:, 0], equal_nan=True)
    if count == 257:
        grid = _d(q[:256]).reshape(16, 16, 3)
        got = radfoam.locate_tets(_d(m["points"]), _table(m["tets"], torch.uint32), _table(m["tet_adjacency"], torch.uint32),
                                  grid, start=torch.zeros((16, 16), dtype=torch.int64, device=DEV))
        assert got.tet.shape == (16, 16) and np.array_equal(got.tet.cpu().numpy().reshape(-1), host["tet"][:256])
        field = radfoam.interpolate(_d(m["points"]), _table(m["tets"], torch.int64), _d(values), grid, got.tet)
        assert field.value.shape == (16, 16) and field.weights.shape == (16, 16, 4) and field.gradient.shape == (16, 16, 3)
        assert np.array_equal(field.weights.cpu().numpy().reshape(-1, 4), want["weights"][:256], equal_nan=True)


@pytest.mark.parametrize("kind,n", MESHES)
@pytest.mark.parametrize("channels", [1, 3, 8])
def test_interpolation_equals_the_host_build(kind, n, channels):
    import radfoam
    m, q = R.mesh(kind, n), R.queries(kind, n)["q"]
    tet = H.walk(m["points"], m["tets"], m["tet_adjacency"], q, R.nearest_start(m, q))["tet"]
    rng = np.random.default_rng(channels)
    values, up = rng.normal(size=(n, channels)).astype(np.float32), rng.normal(size=(len(q), channels))
    want, back = H.interpolate(m["points"], m["tets"], values, q, tet), H.interpolate_grad(m["points"], m["tets"], values, q, tet, up)
    for dtype in (torch.uint32, torch.uint32, torch.int32, torch.int64, "misaligned"):
        args = (_d(m["points"]), _table(m["tets"], dtype), _d(values), _d(q), _d(tet))
        got = radfoam.interpolate(*args)
        assert got.value.shape == (len(q), channels) and got.gradient.shape == (len(q), channels, 3)
        for name in ("value", "weights", "gradient"):
            assert np.array_equal(getattr(got, name).cpu().numpy(), want[name], equal_nan=True), (name, dtype)
        gp, gv, gq = radfoam.interpolate_grad(*args, _d(up))
        assert np.array_equal(gp.cpu().numpy(), back["grad_points"]) and np.array_equal(gv.cpu().numpy(), back["grad_values"])
        assert np.array_equal(gq.cpu().numpy(), back["grad_queries"])


def test_nine_channels_take_the_restatement():
    import radfoam
    m, q = R.mesh("uniform", 400), R.queries("uniform", 400)["q"]
    tet = H.walk(m["points"], m["tets"], m["tet_adjacency"], q)["tet"]
    values = np.random.default_rng(9).normal(size=(400, 9)).astype(np.float32)
    args = (_d(m["points"]), _table(m["tets"], torch.uint32), _d(values), _d(q), _d(tet))
    got = radfoam.interpolate(*args)
    want = H.interpolate(m["points"], m["tets"], values, q, tet)
    assert np.array_equal(got.value.cpu().numpy(), want["value"], equal_nan=True)
    assert np.array_equal(got.weights.cpu().numpy(), want["weights"], equal_nan=True)
    with pytest.raises(RuntimeError, match="at most 8 channels"):
        radfoam.interpolate(*args, backend="hip")


def test_errors_raise_as_on_the_host_and_leave_nothing_behind():
    m = R.mesh("uniform", 400)
    valid = R.queries_of(m)
    want = H.walk(m["points"], m["tets"], m["tet_adjacency"], valid)
    for name, (rows, adj, start, q) in R.malformed(m).items():
        host = H.walk(m["points"], rows, adj, q, start)
        first = int(np.nonzero(host["tet"] < -1)[0][0])
        for dtype in (torch.int64, torch.int32):
            with pytest.raises(RuntimeError, match=f"locate_tets: query {first}:"):
                _locate(m, q, start, dtype, tets=rows, adjacency=adj)
            tet, hops = _locate(m, valid)
            assert np.array_equal(tet, want["tet"]) and np.array_equal(hops, want["hops"]), name


def test_hop_cap_raises_and_does_not_hang():
    m, q = R.mesh("uniform", 400), R.queries("uniform", 400)["q"]
    host = H.walk(m["points"], m["tets"], m["tet_adjacency"], q, max_hops=2)
    first = int(np.nonzero(host["tet"] < -1)[0][0])
    with pytest.raises(RuntimeError, match=f"query {first}: its walk would cross more than max_hops = 2"):
        _locate(m, q, max_hops=2)
    whole = H.walk(m["points"], m["tets"], m["tet_adjacency"], q)["tet"]
    busiest = int(np.bincount(whole[whole >= 0]).argmax())
    with pytest.raises(RuntimeError, match="max_hops"):                # a negatively oriented row: the walk goes round
        _locate(m, q, tets=R.swapped(m, busiest))
    assert np.array_equal(_locate(m, q)[0], whole)


def test_triangulation_locate_and_an_incremental_rebuild():
    import radfoam
    from radfoam_amd.scene_ops import nearest_point
    from tests import tets_ref
    pts = torch.from_numpy(tets_ref.uniform(5001, seed=31)).to(DEV)
    tri = radfoam.Triangulation(pts)
    rng = np.random.default_rng(32)
    q = np.concatenate([rng.uniform(-1.1, 1.1, (400, 3)), [[np.nan, 0, 0], [0, np.inf, 0]]]).astype(np.float32)

    def check():
        p = tri._points
        got = tri.locate(_d(q))
        nearest = nearest_point(p, _d(q[:400])).view(torch.int32).to(torch.int64)   # the tree's answer, by brute force
        start = torch.cat([tri.vert_to_tet().view(torch.int32).to(torch.int64)[nearest],
                           torch.zeros(2, dtype=torch.int64, device=DEV)])
        own = radfoam.locate_tets(p, tri.tets(), tri.tet_adjacency(), _d(q), start=start)
        assert torch.equal(got.tet, own.tet) and torch.equal(got.hops, own.hops)
        tet = got.tet.cpu().numpy()
        assert (tet[400:] == -1).all() and (got.hops.cpu().numpy()[400:] == 0).all()
        m = dict(points=p.cpu().numpy(), tets=tri.tets().cpu().numpy().astype(np.int64))
        R.check_located(m, q, tet)
        host = H.walk(m["points"], m["tets"], tri.tet_adjacency().cpu().numpy(), q, start.cpu().numpy())
        assert np.array_equal(tet, host["tet"]) and np.array_equal(got.hops.cpu().numpy(), host["hops"])
        return got

    first = check()
    tree = tri._tree
    assert tree is not None and tri.locate(_d(q)).tet.equal(first.tet) and tri._tree is tree   # kept, not built again
    gen = torch.Generator().manual_seed(33)
    moved = (tri._points.cpu() + 0.02 * torch.randn((5001, 3), generator=gen)).to(DEV)
    assert tri.rebuild(moved, incremental=True) is False
    assert tri._tree is None and tri._tets is None                      # dropped together
    second = check()
    assert not torch.equal(first.tet, second.tet)


def test_float32_autograd_equals_the_torch_backends():
    import radfoam
    m, q = R.mesh("clustered", 400), R.queries("clustered", 400)["q"]
    tet = H.walk(m["points"], m["tets"], m["tet_adjacency"], q, R.nearest_start(m, q))["tet"]
    rng = np.random.default_rng(12)
    values, up = rng.normal(size=(400, 3)).astype(np.float32), rng.normal(size=(len(q), 3))
    inside = _d(tet >= 0)
    grads = {}
    for backend in ("hip", "torch"):
        leaves = [_d(m["points"]).requires_grad_(), _d(values).requires_grad_(), _d(q).requires_grad_()]
        out = radfoam.interpolate(leaves[0], _table(m["tets"], torch.uint32), leaves[1], leaves[2], _d(tet), backend=backend)
        assert not out.weights.requires_grad and not out.gradient.requires_grad
        (out.value[inside] * _d(up)[inside]).sum().backward()
        grads[backend] = [leaf.grad for leaf in leaves] + [out.value.detach()]
        assert all(g.dtype == torch.float32 for g in grads[backend][:3])
    # both evaluate the spelled order in double; the device's torch may round a step differently and index_add_ adds in
    # any order: the bounds of the CPU tests (either side within them of the exact result), and one float32 rounding
    mine, theirs = grads["hip"][3].cpu().numpy(), grads["torch"][3].cpu().numpy()
    assert np.array_equal(np.isnan(mine), np.isnan(theirs)) and np.array_equal(np.isnan(mine).any(1), tet < 0)
    magnitude = float(np.abs(values).max())
    for k in np.nonzero(tet >= 0)[0]:
        assert (np.abs(mine[k] - theirs[k]) <= 2 * R.value_tolerance(m["points"], m["tets"][tet[k]], q[k], magnitude)).all(), k
    tols = R.autograd_tolerances(m, q, tet, values, up)
    for mine, theirs, tol in zip(grads["hip"][:3], grads["torch"][:3], tols):
        err = (mine.double() - theirs.double()).abs().cpu().numpy()
        assert (err <= tol[:, None] + 2.0 ** -23 * theirs.abs().cpu().numpy()).all()


def test_isosurface_vertices_interpolate_back_to_the_level():
    import radfoam
    from tests import tets_ref
    pts = torch.from_numpy(tets_ref.uniform(2000, seed=22)).to(DEV)
    tri = radfoam.Triangulation(pts)
    p = tri._points
    values = (0.6 - p.to(torch.float64).norm(dim=1)).to(torch.float32)
    level = 0.05
    mesh = radfoam.isosurface(p, tri.tets(), values, level)
    x64 = mesh.vertices.detach()
    q = x64.to(torch.float32)
    where = tri.locate(q)
    assert (where.tet >= 0).all()
    field = radfoam.interpolate(p, tri.tets(), values, q, where.tet)
    value, grad = field.value.cpu().numpy(), field.gradient.cpu().numpy()
    m = dict(points=p.cpu().numpy(), tets=tri.tets().cpu().numpy().astype(np.int64))
    R.check_located(m, q.cpu().numpy()[::50], where.tet.cpu().numpy()[::50])
    # the field is linear in the located tetrahedron, which holds the vertex's edge: f(q) = level + g . (q - x) for the exact
    # vertex x; the computed vertex is within 4 roundings of it, q one float32 rounding further
    x, qn, tet = x64.cpu().numpy(), q.cpu().numpy(), where.tet.cpu().numpy()
    moved = (np.abs(grad) * (np.abs(qn.astype(np.float64) - x) + 4 * R.U * np.abs(x))).sum(1)
    magnitude, worst = float(values.abs().max()), 0.0
    for k in range(0, len(qn), 7):
        tol = R.value_tolerance(m["points"], m["tets"][tet[k]], qn[k], magnitude) + 2 * moved[k]
        worst = max(worst, abs(value[k] - level) / tol)
        assert abs(value[k] - level) <= tol, (k, value[k], tol)
    print(f"isosurface vertices back to the level: worst {worst:.3g} of the bound")
