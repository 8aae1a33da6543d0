"""radfoam.locate_tets / interpolate / interpolate_grad without a GPU: the numpy / torch restatement of
radfoam_amd/locate.py and the host build of csrc/rf_locate.hpp (tests/host_harness/locate_host.cpp) against each other and
against Fractions of the float32 inputs (tests/locate_ref.py), on Qhull meshes."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import radfoam
from radfoam_amd import locate as L
from tests import locate_ref as R
from tests.host_harness import locate_host as H


def _t(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t if dtype is None else t.to(dtype)


def _locate(m, q, start=None, max_hops=None, tets=None, adjacency=None):
    got = radfoam.locate_tets(_t(m["points"]), _t(m["tets"] if tets is None else tets),
                              _t(m["tet_adjacency"] if adjacency is None else adjacency), _t(q),
                              start=None if start is None else _t(start), max_hops=max_hops)
    assert got.tet.dtype == torch.int64 and got.hops.dtype == torch.int32 and got.tet.shape == q.shape[:-1]
    return got.tet.numpy(), got.hops.numpy()


@pytest.mark.parametrize("kind,n", R.MESHES)
def test_walk_contains_its_query_and_minus_one_is_outside(kind, n):
    m, qs = R.mesh(kind, n), R.queries(kind, n)
    q = qs["q"]
    on_mesh = slice(300, 320 + qs["mids"])                                                   # sites and edge midpoints
    assert qs["mids"] >= 10
    near = R.nearest_start(m, q)
    results = []
    for start in (None, near):
        tet, hops = _locate(m, q, start)
        host = H.walk(m["points"], m["tets"], m["tet_adjacency"], q, start)
        assert np.array_equal(tet, host["tet"]) and np.array_equal(hops, host["hops"])      # the backends, element for element
        R.check_located(m, q, tet)
        assert tet[qs["nan"]] == -1 and hops[qs["nan"]] == 0
        assert (tet[-11:-1] == -1).all()                                                     # the queries far outside
        print(f"{kind} {n} start={'row 0' if start is None else 'nearest site'}: at most {hops.max()} hops, "
              f"{host['exact']} of {host['predicates']} predicates left the fp64 filter")
        results.append(tet)
    assert (results[0][on_mesh] >= 0).all() and (results[1][on_mesh] >= 0).all()
    for k in range(len(q) - 1):
        if results[0][k] >= 0 and R.strictly_inside(m["points"], m["tets"][results[0][k]], q[k]):
            assert results[0][k] == results[1][k], k
    assert ((results[0] >= 0) == (results[1] >= 0)).all()


def test_index_dtypes_and_query_shapes():
    m, q = R.mesh("uniform", 400), R.queries("uniform", 400)["q"][:360]
    want, hops = _locate(m, q)
    for dtype in (torch.int32, torch.int64):
        got = radfoam.locate_tets(_t(m["points"]), _t(m["tets"], dtype), _t(m["tet_adjacency"], dtype), _t(q))
        assert np.array_equal(got.tet.numpy(), want) and np.array_equal(got.hops.numpy(), hops)
    as_u32 = lambda x: _t(x.astype(np.int64).astype(np.uint32))
    got = radfoam.locate_tets(_t(m["points"]), as_u32(m["tets"]), as_u32(m["tet_adjacency"]), _t(q).reshape(6, 60, 3),
                              start=torch.zeros((6, 60), dtype=torch.int32))
    assert got.tet.shape == (6, 60) and np.array_equal(got.tet.numpy().reshape(-1), want)
    host = H.walk(m["points"], m["tets"].astype(np.uint32), m["tet_adjacency"].astype(np.int64).astype(np.uint32), q)
    assert np.array_equal(host["tet"], want) and np.array_equal(host["hops"], hops)
    empty = radfoam.locate_tets(_t(m["points"]), _t(m["tets"]), _t(m["tet_adjacency"]), torch.zeros((0, 3)))
    assert empty.tet.shape == (0,) and empty.hops.shape == (0,)


def test_hop_cap_raises():
    m, q = R.mesh("uniform", 400), R.queries("uniform", 400)["q"]
    _, hops = _locate(m, q)
    first = int(np.nonzero(hops > 2)[0][0])
    with pytest.raises(RuntimeError, match=f"query {first}: its walk would cross more than max_hops = 2"):
        _locate(m, q, max_hops=2)
    host = H.walk(m["points"], m["tets"], m["tet_adjacency"], q, max_hops=2)
    capped = host["tet"] < -1
    assert np.array_equal(capped, hops > 2) and ((-2 - host["tet"][capped]) & 7 == 4).all() and (host["hops"][capped] == 2).all()
    kept = ~capped
    assert np.array_equal(host["tet"][kept], _locate(m, q)[0][kept])


def test_malformed_tables_raise_and_the_next_call_is_right():
    m = R.mesh("uniform", 400)
    valid_q = R.queries_of(m)
    want = _locate(m, valid_q)
    kinds = {"above": 0, "below": 0, "adjacency": 1, "flat": 2, "start": 3}
    for name, (rows, adj, start, q) in R.malformed(m).items():
        with pytest.raises(RuntimeError, match="locate_tets: query"):
            _locate(m, q, start, tets=rows, adjacency=adj)
        host = H.walk(m["points"], rows, adj, q, start)
        faulted = host["tet"][host["tet"] < -1]
        seen = set(((-2 - faulted) & 7).tolist())                       # a flat row may also send a walk round to the cap
        assert kinds[name] in seen and seen <= {kinds[name], 4 if name == "flat" else kinds[name]}, name
        tet, hops = L._walk_numpy(m["points"], rows, adj, q, np.zeros(len(q), dtype=np.int64) if start is None else start,
                                  len(rows))
        assert np.array_equal(tet, host["tet"]) and np.array_equal(hops, host["hops"]), name
        again = _locate(m, valid_q)
        assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1])


def test_a_negatively_oriented_row_is_never_returned():
    m, q = R.mesh("uniform", 400), R.queries("uniform", 400)["q"]
    tet, _ = _locate(m, q)
    t = int(np.bincount(tet[tet >= 0]).argmax())                       # a row that holds queries
    rows = R.swapped(m, t)
    for start in (None, R.nearest_start(m, q), np.full(len(q), t, dtype=np.int64)):
        host = H.walk(m["points"], rows, m["tet_adjacency"], q, start)
        s = np.zeros(len(q), dtype=np.int64) if start is None else start
        mine = L._walk_numpy(m["points"], rows, m["tet_adjacency"], q, s, len(rows))
        assert np.array_equal(mine[0], host["tet"]) and np.array_equal(mine[1], host["hops"])
        assert not (host["tet"] == t).any()
        for k in np.nonzero(host["tet"] >= 0)[0]:
            assert R.contains(m["points"], rows[host["tet"][k]], q[k])
    with pytest.raises(RuntimeError, match="max_hops"):
        _locate(m, q, tets=rows)


# ---- interpolation ------------------------------------------------------------------------------------------------------

FIELDS = [("uniform", 400), ("clustered", 400)]
_FIELD = {}


def _field(kind, n):
    """the mesh, its queries and where they are, computed once"""
    if (kind, n) not in _FIELD:
        m, q = R.mesh(kind, n), R.queries(kind, n)["q"]
        tet, _ = _locate(m, q, R.nearest_start(m, q))
        _FIELD[(kind, n)] = (m, q, tet)
    return _FIELD[(kind, n)]


def _interpolate(m, values, q, tet, backend=None):
    return radfoam.interpolate(_t(m["points"]), _t(m["tets"]), _t(values), _t(q), _t(tet), backend=backend)


@pytest.mark.parametrize("kind,n", FIELDS)
def test_weights_agree_with_the_exact_rational_weights(kind, n):
    m, q, tet = _field(kind, n)
    values = np.random.default_rng(3).normal(size=n).astype(np.float32)
    got = _interpolate(m, values, q, tet)
    host = H.interpolate(m["points"], m["tets"], values, q, tet)
    w = got.weights.numpy()
    assert got.value.shape == (len(q),) and w.shape == (len(q), 4) and got.gradient.shape == (len(q), 3)
    assert np.array_equal(w, host["weights"], equal_nan=True)
    assert np.array_equal(got.value.numpy(), host["value"][:, 0], equal_nan=True)
    assert np.array_equal(got.gradient.numpy(), host["gradient"][:, 0], equal_nan=True)
    worst = 0.0
    for k in range(len(q)):
        if tet[k] < 0:
            assert np.isnan(w[k]).all() and np.isnan(host["value"][k]).all() and np.isnan(host["gradient"][k]).all()
            continue
        exact = R.exact_weights(m["points"], m["tets"][tet[k]], q[k])
        tol = R.weight_tolerances(m["points"], m["tets"][tet[k]], q[k], w[k])
        err = np.array([abs(float(exact[i] - R.Fraction(float(w[k, i])))) for i in range(4)])
        worst = max(worst, (err[tol > 0] / tol[tol > 0]).max(initial=0.0))
        assert (err <= tol).all(), (k, err, tol)
    print(f"{kind} {n}: worst weight error {worst:.3g} of its bound")


@pytest.mark.parametrize("kind,n", FIELDS)
def test_a_linear_field_is_reproduced(kind, n):
    m, q, tet = _field(kind, n)
    a, b = np.array([0.7, -1.3, 0.4]), 0.25
    values = m["points"].astype(np.float64) @ a + b
    got = _interpolate(m, values, q, tet)
    host = H.interpolate(m["points"], m["tets"], values, q, tet)
    assert np.array_equal(got.value.numpy(), host["value"][:, 0], equal_nan=True)
    magnitude, worst = np.abs(values).max(), 0.0
    for k in np.nonzero(tet >= 0)[0]:
        exact = sum(R.Fraction(float(q[k, d])) * R.Fraction(float(a[d])) for d in range(3)) + R.Fraction(float(b))
        # the values themselves are rounded once from the exact field: within u * magnitude each, convexly combined
        tol = R.value_tolerance(m["points"], m["tets"][tet[k]], q[k], magnitude) + 4 * R.U * magnitude
        err = abs(float(exact - R.Fraction(float(got.value[k]))))
        worst = max(worst, err / tol)
        assert err <= tol, (k, err, tol)
    print(f"{kind} {n}: worst value error {worst:.3g} of its bound")


@pytest.mark.parametrize("channels", [1, 3, 8])
def test_gradient_parts_equal_the_host_builds_bit_for_bit(channels):
    m, q, tet = _field("clustered", 400)
    rng = np.random.default_rng(4)
    values = rng.normal(size=(400, channels)).astype(np.float32)
    up = rng.normal(size=(len(q), channels))
    gp, gv, gq = radfoam.interpolate_grad(_t(m["points"]), _t(m["tets"]), _t(values), _t(q), _t(tet), _t(up))
    host = H.interpolate_grad(m["points"], m["tets"], values, q, tet, up)
    parts = L._grad_parts_torch(_t(m["points"]), _t(m["tets"]), _t(values), _t(q), _t(tet), _t(up))[0]
    assert np.array_equal(parts.numpy(), host["parts"])
    assert np.array_equal(gp.numpy(), host["grad_points"]) and np.array_equal(gv.numpy(), host["grad_values"])
    assert np.array_equal(gq.numpy(), host["grad_queries"])
    assert (host["parts"][tet < 0] == 0).all() and (host["grad_queries"][tet < 0] == 0).all()
    nine = rng.normal(size=(400, 9)).astype(np.float32)                 # wider than the kernels: the restatement
    wide = _interpolate(m, nine, q, tet)
    assert wide.value.shape == (len(q), 9) and wide.gradient.shape == (len(q), 9, 3)
    assert np.array_equal(wide.value.numpy(), H.interpolate(m["points"], m["tets"], nine, q, tet)["value"], equal_nan=True)


@pytest.mark.parametrize("kind,n", FIELDS)
def test_autograd_agrees_with_float64_autograd_of_the_restatement(kind, n):
    m, q, tet = _field(kind, n)
    rng = np.random.default_rng(6)
    values = rng.normal(size=(n, 3)).astype(np.float32)
    up = rng.normal(size=(len(q), 3))
    leaves = [_t(m["points"]).requires_grad_(), _t(values).requires_grad_(), _t(q).requires_grad_()]
    out = radfoam.interpolate(leaves[0], _t(m["tets"]), leaves[1], leaves[2], _t(tet))
    assert not out.weights.requires_grad and not out.gradient.requires_grad
    inside = _t(tet >= 0)
    (out.value[inside] * _t(up)[inside]).sum().backward()
    closed = radfoam.interpolate_grad(leaves[0], _t(m["tets"]), leaves[1], leaves[2], _t(tet), _t(up))
    for leaf, grad in zip(leaves, closed):                             # the autograd.Function hands out interpolate_grad
        assert leaf.grad.dtype == torch.float32 and torch.equal(leaf.grad, grad.to(torch.float32))
    assert (closed[2][~inside] == 0).all()
    # the reference: autograd through the restatement in double, over the located queries alone (a NaN row poisons it)
    ref = [_t(m["points"]).double().requires_grad_(), _t(values).double().requires_grad_(),
           _t(q).double()[inside].requires_grad_()]
    value = L._forward_torch(ref[0], _t(m["tets"]), ref[1], ref[2], _t(tet)[inside])[0]
    (value * _t(up)[inside]).sum().backward()
    closed = (closed[0], closed[1], closed[2][inside])
    tol_p, tol_v, tol_q = R.autograd_tolerances(m, q, tet, values, up)
    tol_q = tol_q[tet >= 0]
    worst = 0.0
    for name, mine, theirs, tol in (("points", closed[0], ref[0].grad, tol_p[:, None]), ("values", closed[1], ref[1].grad, tol_v[:, None]),
                                    ("queries", closed[2], ref[2].grad, tol_q[:, None])):
        err = (mine - theirs).abs().numpy()
        scale = theirs.abs().max().item()
        print(f"{kind} {n} grad {name}: worst difference {err.max():.3g} ({err.max() / scale:.3g} of the largest entry)")
        hit = tol > 0
        worst = max(worst, (err / np.where(hit, tol, 1.0))[np.broadcast_to(hit, err.shape)].max())
        assert (err <= tol).all(), name
    print(f"{kind} {n}: worst difference {worst:.3g} of its bound")


def test_difference_quotient_in_points():
    m = R.mesh("uniform", 400)
    pts, rows = m["points"], m["tets"]
    p64 = pts.astype(np.float64)[rows]
    vol = np.abs(np.einsum("ij,ij->i", p64[:, 1] - p64[:, 0], np.cross(p64[:, 2] - p64[:, 0], p64[:, 3] - p64[:, 0])))
    t = int(vol.argmax())
    q = (p64[t] * np.array([0.4, 0.3, 0.2, 0.1])[:, None]).sum(0).astype(np.float32)[None]
    assert R.strictly_inside(pts, rows[t], q[0])
    tet = np.array([t], dtype=np.int64)
    values = np.random.default_rng(8).normal(size=400).astype(np.float32)
    gp = radfoam.interpolate_grad(_t(pts), _t(rows), _t(values), _t(q), _t(tet), torch.ones(1))[0].numpy()
    assert (gp[np.setdiff1d(np.arange(400), rows[t])] == 0).all()
    # central differences of a function rational in the corner: the truncation is of relative order (h / height)^2;
    # h = 1e-4 of the cube root of the volume, the largest tetrahedron of a uniform cloud is no sliver: 1e-5 is ample
    h = 1e-4 * vol[t] ** (1 / 3)
    field = lambda p: float(L._forward_torch(_t(p), _t(rows), _t(values).double()[:, None], _t(q).double(), _t(tet))[0])
    scale = np.abs(gp[rows[t]]).max()
    for s in rows[t]:
        for d in range(3):
            up, down = pts.astype(np.float64), pts.astype(np.float64)
            up[s, d] += h
            down[s, d] -= h
            quotient = (field(up) - field(down)) / (2 * h)
            assert abs(quotient - gp[s, d]) <= 1e-5 * scale, (s, d, quotient, gp[s, d])
