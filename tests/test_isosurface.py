"""Marching tetrahedra on the Delaunay mesh, the part that runs without a GPU: the torch backend of radfoam.isosurface,
isosurface_vertices and isosurface_vertices_grad, and radfoam_amd/csrc/rf_iso.hpp compiled for the host
(tests/host_harness/iso_host), against the table-free reference of tests/isosurface_ref.py, the topology of a closed
surface, a linear field, difference quotients and autograd.  tests/test_gpu_isosurface.py holds the device to them.

The clouds are default_rng(seed).uniform(-1, 1, (n, 3)) in float32 under scipy's Delaunay with values = 0.6 - |p| at level
0 (iso_host.CLOUDS lists the tetrahedra, vertices and triangles counted when the feature was proposed).

Bounds.  Linear field in float64: the vertex solves n.x + c = level exactly in exact arithmetic, the bound 1e-14 max|v| is
a few dozen roundings of the largest value.  With float32 values the residual is (1 - t) (v_a - fl(v_a)) + t (v_b - fl(v_b)),
t in [0,1], so at most one rounding 2^-24 max|v| of an input, plus the float64 bound.  Difference quotients: central
quotients at h and h/2 along random directions, extrapolated; the miss is held to the extrapolated-away truncation term
|Q(h) - Q(h/2)| plus the rounding 4 eps sum|terms of L| / h of the quotient itself.

Measured on the host: area vectors against the reference at most 2.5e-16 of the largest on the four clouds and on the
16-mask pair; linear field 1.1e-16 max|v| in float64 and 0.25 * 2^-24 max|v| with float32 values; difference quotients,
worst miss over 12 directions 0.031 of the bound; isosurface_vertices_grad against plain autograd 7.8e-16 (points) and
1.6e-15 (values) of max(1, |row|); host build against torch: keys, triangles, vertices, t and backward parts bit-equal
on all four clouds and the mask pair."""
import math
import os

import numpy as np
import pytest
import torch

from tests import isosurface_ref as R
from tests.host_harness import iso_host as HI

CLOUDS = tuple(HI.CLOUDS)
F64 = torch.float64


def _np(mesh):
    return {k: getattr(mesh, k).detach().cpu().numpy() for k in mesh._fields}


def _torch_mesh(c, level=0.0, **kw):
    import radfoam

    return radfoam.isosurface(torch.from_numpy(c["points"]), torch.from_numpy(c["tets"]), torch.from_numpy(c["values"]),
                              level, **kw)


def _check_against_reference(got, points, tets, values, level, label):
    """key sets equal, area vectors to 1e-12 of the largest"""
    sets, areas = R.reference(points, tets, values, level)
    assert HI.key_sets(got, len(tets)) == sets
    mine = HI.area_vectors(got, len(tets))
    worst = np.abs(mine - areas).max() / max(np.abs(areas).max(), 1e-300)
    print(f"{label}: max |area vector - reference| = {worst:.3g} of the largest")
    assert worst <= 1e-12
    return sets


def test_public_names_sources_and_abi_conventions():
    import radfoam
    import radfoam_amd
    from radfoam_amd import _lib, build

    for name in ("IsoMesh", "isosurface", "isosurface_vertices", "isosurface_vertices_grad"):
        assert name in radfoam.__all__ and name in radfoam_amd.__all__ and hasattr(radfoam, name)
    assert radfoam.IsoMesh._fields == ("vertices", "vertex_sites", "vertex_t", "triangles", "triangle_tet")
    names = lambda paths: {os.path.basename(p) for p in paths}
    assert "rf_isosurface.hip" in names(build.EXTRA_SOURCES)
    assert {"rf_iso.hpp", "radfoam_hip_isosurface.h"} <= names(build.EXTRA_HEADERS)
    assert not names(build.SOURCES + build.HEADERS) & {"rf_isosurface.hip", "rf_iso.hpp", "radfoam_hip_isosurface.h"}
    lib = _lib.load()
    for name in ("rf_isosurface_count", "rf_isosurface_emit", "rf_isosurface_vertices", "rf_isosurface_vertices_grad"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.rf_isosurface_count(None, 4, 0, None, 0, 0.0, None, None, None) == 0            # nothing to do
    assert lib.rf_isosurface_count(None, 4, 5, None, 3, 0.0, None, None, None) == -1
    assert "null pointer" in _lib.last_error()
    dummy = np.zeros(64).ctypes.data
    assert lib.rf_isosurface_count(dummy, 2, 5, dummy, 3, 0.0, dummy, dummy, None) == -1
    assert "index_bytes" in _lib.last_error()
    assert lib.rf_isosurface_count(dummy + 8, 4, 5, dummy, 3, 0.0, dummy, dummy, None) == -1
    assert "aligned" in _lib.last_error()
    assert lib.rf_isosurface_emit(None, 4, 0, None, None, 0, 0.0, None, None, 0, None, None, None) == 0
    assert lib.rf_isosurface_emit(None, 8, 5, None, None, 3, 0.0, None, None, 4, None, None, None) == -1
    assert "null pointer" in _lib.last_error()
    assert lib.rf_isosurface_vertices(None, None, 0, None, 0, 0.0, None, None, None) == 0
    assert lib.rf_isosurface_vertices(None, None, 5, None, 3, 0.0, None, None, None) == -1
    assert lib.rf_isosurface_vertices_grad(None, None, 0, None, 0, 0.0, *([None] * 7)) == 0
    assert lib.rf_isosurface_vertices_grad(None, None, 5, None, 3, 0.0, *([None] * 7)) == -1
    assert "null pointer" in _lib.last_error()


def test_input_checks_without_a_device():
    import radfoam

    pts, val = torch.zeros(10, 3), torch.zeros(10)
    tets, sites = torch.zeros((2, 4), dtype=torch.int64), torch.zeros((2, 2), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="float32 CUDA points"):
        radfoam.isosurface(pts, tets, val, 0.0, backend="hip")
    with pytest.raises(RuntimeError, match="float32 CUDA points"):
        radfoam.isosurface_vertices(pts, val, sites, 0.0, backend="hip")
    with pytest.raises(ValueError, match="backend must be"):
        radfoam.isosurface(pts, tets, val, 0.0, backend="triton")
    for bad in (pts[:, :2], pts.long(), pts.reshape(-1)):
        with pytest.raises(RuntimeError, match="points must be"):
            radfoam.isosurface(bad, tets, val, 0.0)
    for bad in (val[:9], val.long(), val[:, None], None):
        with pytest.raises(RuntimeError, match="values must be"):
            radfoam.isosurface(pts, tets, bad, 0.0)
    for bad in (tets.to(torch.int16), tets[:, :3], tets.reshape(-1), tets.double(), None):
        with pytest.raises(RuntimeError, match="tets must be"):
            radfoam.isosurface(pts, bad, val, 0.0)
    for bad in (sites.int(), sites[:, :1], sites.reshape(-1)):
        with pytest.raises(RuntimeError, match="vertex_sites must be"):
            radfoam.isosurface_vertices(pts, val, bad, 0.0)
    for bad in (torch.zeros(2, 3, dtype=torch.int64), torch.zeros(3, 3), None):
        with pytest.raises(RuntimeError, match="grad_vertices must be"):
            radfoam.isosurface_vertices_grad(pts, val, sites, 0.0, bad)
    assert radfoam.isosurface_vertices(pts, val, sites[:0], 0.0).shape == (0, 3)
    gp, gv = radfoam.isosurface_vertices_grad(pts, val, sites[:0], 0.0, torch.zeros(0, 3))
    assert gp.shape == (10, 3) and gv.shape == (10,) and gp.dtype == gv.dtype == F64


@pytest.mark.parametrize("mask", range(16))
def test_all_sixteen_masks_on_both_orientations(mask):
    import radfoam

    level = 0.25
    pts, tets = HI.mask_pair()
    values = HI.mask_values(mask, level)
    inside = bin(mask).count("1")
    want = {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[inside]
    got = _np(radfoam.isosurface(torch.from_numpy(pts), torch.from_numpy(tets), torch.from_numpy(values), level))
    host = HI.mesh(pts, tets, values, level)
    for m, label in ((got, "torch"), (host, "host build")):
        assert np.array_equal(np.bincount(m["triangle_tet"], minlength=2), [want, want]), label
        if want == 0:
            assert len(m["vertices"]) == 0 and len(m["triangles"]) == 0
            continue
        sets = _check_against_reference(m, pts, tets, values, level, f"mask {mask} {label}")
        assert sets[0] == sets[1] and len(sets[0]) == (4 if want == 2 else 3)
        assert len(m["vertices"]) == len(sets[0])                     # the two tetrahedra share every vertex
        x = m["vertices"][m["triangles"]]
        a = np.cross(x[:, 1] - x[:, 0], x[:, 2] - x[:, 0])
        assert np.allclose(a[:want].sum(0), a[want:].sum(0), rtol=0, atol=1e-14)    # the same surface from either row order
    for key in got:
        assert np.array_equal(got[key], host[key]), key


@pytest.mark.parametrize("n,seed", CLOUDS)
def test_level_set_of_a_ball_is_closed_oriented_and_of_genus_zero(n, seed):
    c = HI.cloud(n, seed)
    nt, nv, nf = HI.CLOUDS[(n, seed)]
    got = _np(_torch_mesh(c))
    assert len(c["tets"]) == nt and got["vertices"].shape == (nv, 3) and got["triangles"].shape == (nf, 3)
    assert got["vertices"].dtype == np.float64 and got["vertex_t"].dtype == np.float64
    assert all(got[k].dtype == np.int64 for k in ("vertex_sites", "triangles", "triangle_tet"))
    assert HI.check_closed(got, f"({n}, {seed})") == (nv, 3 * nf // 2, nf)
    volume, ball = HI.enclosed_volume(got), 4.0 / 3.0 * math.pi * HI.RADIUS ** 3
    print(f"({n}, {seed}): enclosed volume {volume:.6f} of the ball's {ball:.6f}")
    assert 0.0 < volume < ball
    _check_against_reference(got, c["points"], c["tets"], c["values"], 0.0, f"({n}, {seed})")
    sites = got["vertex_sites"]
    assert (sites[:, 0] < sites[:, 1]).all() and sites.min() >= 0 and sites.max() < n
    packed = sites[:, 0] * 2 ** 32 + sites[:, 1]
    assert (np.diff(packed) > 0).all()                                # ascending and unique
    assert (np.diff(got["triangle_tet"]) >= 0).all()
    assert set(np.bincount(got["triangle_tet"]).tolist()) == {0, 1, 2}    # both case kinds occur
    assert ((got["vertex_t"] >= 0) & (got["vertex_t"] <= 1)).all()
    p = c["points"].astype(np.float64)
    lerp = p[sites[:, 0]] + got["vertex_t"][:, None] * (p[sites[:, 1]] - p[sites[:, 0]])
    assert np.array_equal(lerp, got["vertices"])                      # vertex_t interpolates the sites to the vertices


def test_linear_field_in_float64_and_with_float32_values():
    import radfoam

    c = HI.cloud(400, 1)
    p = torch.from_numpy(c["points"]).to(F64)
    normal, offset, level = torch.tensor([0.3, -0.5, 0.8], dtype=F64), 0.05, 0.1
    values = p @ normal + offset
    vmax = float(values.abs().max())
    tets = torch.from_numpy(c["tets"])
    mesh = radfoam.isosurface(p, tets, values, level)
    assert mesh.vertices.size(0) > 50
    residual = float((mesh.vertices @ normal + offset - level).abs().max())
    print(f"linear field, float64: max |n.x + c - level| = {residual / vmax:.3g} max|v|")
    assert residual <= 1e-14 * vmax
    rounded = values.to(torch.float32)
    mesh32 = radfoam.isosurface(p, tets, rounded, level)
    residual32 = float((mesh32.vertices @ normal + offset - level).abs().max())
    print(f"linear field, float32 values: max |n.x + c - level| = {residual32 / (2.0 ** -24 * vmax):.3g} * 2^-24 max|v|")
    assert residual32 <= (2.0 ** -24 + 1e-14) * vmax


def _smooth(x, w):
    return (w * torch.sin(1.3 * x)).sum() + 0.5 * (x * x).sum()


def test_gradients_against_difference_quotients_and_autograd():
    import radfoam

    c = HI.cloud(400, 1)
    p0, v0 = torch.from_numpy(c["points"]).to(F64), torch.from_numpy(c["values"]).to(F64)
    mesh = radfoam.isosurface(p0, torch.from_numpy(c["tets"]), v0, 0.0)
    sites, nv = mesh.vertex_sites, mesh.vertices.size(0)
    gen = torch.Generator().manual_seed(5)
    w = torch.randn((nv, 3), dtype=F64, generator=gen)
    loss = lambda p, v: _smooth(radfoam.isosurface_vertices(p, v, sites, 0.0), w)
    p, v = p0.clone().requires_grad_(True), v0.clone().requires_grad_(True)
    value = loss(p, v)
    value.backward()
    assert torch.isfinite(p.grad).all() and torch.isfinite(v.grad).all()
    with torch.no_grad():
        x = radfoam.isosurface_vertices(p0, v0, sites, 0.0)
        assert torch.equal(x, mesh.vertices.detach())                  # the fixed topology gives the mesh's own vertices
        terms = float((w * torch.sin(1.3 * x)).abs().sum() + 0.5 * (x * x).sum())
        h, worst = 2.0 ** -14, 0.0
        for k in range(12):
            dp = torch.randn(p0.shape, dtype=F64, generator=gen) * (k % 3 != 1) * 0.02      # every third: values alone,
            dv = torch.randn(v0.shape, dtype=F64, generator=gen) * (k % 3 != 2) * 0.02      # the next: points alone
            q = lambda s: float(loss(p0 + s * dp, v0 + s * dv) - loss(p0 - s * dp, v0 - s * dv)) / (2 * s)
            q1, q2 = q(h), q(h / 2)
            want = (4 * q2 - q1) / 3
            mine = float((p.grad * dp).sum() + (v.grad * dv).sum())
            bound = abs(q1 - q2) + 4 * 2.0 ** -52 * terms / (h / 2)
            worst = max(worst, abs(mine - want) / bound)
            assert abs(mine - want) <= bound, (k, mine, want, bound)
    print(f"difference quotients: worst miss {worst:.3g} of the bound")

    # end to end through isosurface itself: both inputs are reached
    p, v = p0.clone().requires_grad_(True), v0.clone().requires_grad_(True)
    radfoam.isosurface(p, torch.from_numpy(c["tets"]), v, 0.0).vertices.sum().backward()
    assert p.grad is not None and v.grad is not None and p.grad.abs().sum() > 0 and v.grad.abs().sum() > 0
    assert torch.isfinite(p.grad).all() and torch.isfinite(v.grad).all()
    # sum_v x_v moves with its sites: every vertex hands its upstream on in full
    assert abs(float(p.grad.sum()) - 3 * nv) <= 1e-12 * 3 * nv

    # the backward operator against plain autograd through the same formula
    g = torch.randn((nv, 3), dtype=F64, generator=gen)
    gp, gv = radfoam.isosurface_vertices_grad(p0, v0, sites, 0.0, g, backend="torch")
    p, v = p0.clone().requires_grad_(True), v0.clone().requires_grad_(True)
    a, b = sites[:, 0], sites[:, 1]
    plain = p[a] + ((0.0 - v[a]) / (v[b] - v[a]))[:, None] * (p[b] - p[a])
    (plain * g).sum().backward()
    for mine, want, label in ((gp, p.grad, "points"), (gv[:, None], v.grad[:, None], "values")):
        miss = ((mine - want).abs().amax(1) / want.abs().amax(1).clamp(min=1.0)).max()
        print(f"isosurface_vertices_grad against autograd, {label}: {float(miss):.3g} of max(1, |row|)")
        assert float(miss) <= 1e-14


def test_edge_cases():
    import radfoam

    c = HI.cloud(64, 0)
    pts, tets, val = torch.from_numpy(c["points"]), torch.from_numpy(c["tets"]), torch.from_numpy(c["values"])
    full = _np(radfoam.isosurface(pts, tets, val, 0.0))

    def is_empty(m):
        assert [tuple(getattr(m, k).shape) for k in m._fields] == [(0, 3), (0, 2), (0,), (0, 3), (0,)]
        assert m.vertices.dtype == m.vertex_t.dtype == F64
        assert m.vertex_sites.dtype == m.triangles.dtype == m.triangle_tet.dtype == torch.int64

    is_empty(radfoam.isosurface(pts, tets[:0], val, 0.0))                            # T = 0
    is_empty(radfoam.isosurface(pts, tets, val, 5.0))                                # no crossing: all outside
    is_empty(radfoam.isosurface(pts, tets, val, -5.0))                               # all inside
    for dtype in (torch.uint32, torch.int32):                                        # the index types give the same mesh
        other = _np(radfoam.isosurface(pts, tets.to(dtype), val, 0.0))
        for key in full:
            assert np.array_equal(other[key], full[key]), (dtype, key)

    # value == level exactly is outside: the same topology, and the vertices of the site's edges sit on it, t = 0 or 1
    is_empty(radfoam.isosurface(pts, tets, val, float(c["values"].max())))           # the largest value is not above itself
    a, b = (int(s) for s in full["vertex_sites"][0])
    on = a if c["values"][a] <= 0.0 else b
    level_valued = val.clone()
    level_valued[on] = 0.0
    m = radfoam.isosurface(pts, tets, level_valued, 0.0)
    assert np.array_equal(m.vertex_sites.numpy(), full["vertex_sites"]) and np.array_equal(m.triangles.numpy(), full["triangles"])
    touching = (m.vertex_sites == on).any(1)
    assert int(touching.sum()) >= 1
    assert torch.equal(m.vertex_t[touching], (m.vertex_sites[touching, 1] == on).to(F64))
    assert torch.equal(m.vertices[touching], pts[on].to(F64).expand(int(touching.sum()), 3))
    HI.check_closed(_np(m), "a site on the level")

    # a NaN value: the tetrahedra around the site are skipped, the rest is unchanged
    site = int(full["vertex_sites"][0, 0])
    holed = val.clone()
    holed[site] = float("nan")
    m = _np(radfoam.isosurface(pts, tets, holed, 0.0))
    around = (c["tets"] == site).any(1)
    keep = ~around[full["triangle_tet"]]
    assert keep.sum() < len(keep) and np.array_equal(m["triangle_tet"], full["triangle_tet"][keep])
    assert not (m["vertex_sites"] == site).any() and np.isfinite(m["vertices"]).all()
    for bad in (float("inf"), float("-inf")):
        holed[site] = bad
        assert np.array_equal(_np(radfoam.isosurface(pts, tets, holed, 0.0))["triangle_tet"], m["triangle_tet"])

    # an index out of range raises and names the first such tetrahedron
    for dtype, index in ((torch.int64, 64), (torch.int64, -1), (torch.int32, -1), (torch.uint32, 64), (torch.int64, 2 ** 40)):
        broken = tets.clone()
        broken[7, 2] = index if dtype != torch.uint32 else 64
        broken[11, 0] = 64
        with pytest.raises(RuntimeError, match=r"tetrahedron 7 has a corner index outside \[0, 64\)"):
            radfoam.isosurface(pts, broken.to(dtype), val, 0.0)

    # a stale topology: v_a == v_b is NaN forward and adds nothing backward; otherwise t extrapolates
    p = pts.to(F64).requires_grad_(True)
    v = torch.linspace(-1.0, 1.0, 64, dtype=F64)
    v[3] = v[2]
    v = v.requires_grad_(True)
    sites = torch.tensor([[2, 3], [0, 1], [4, 70], [5, 9]], dtype=torch.int64)
    x = radfoam.isosurface_vertices(p, v, sites, 0.0)
    assert torch.isnan(x[0]).all() and torch.isnan(x[2]).all() and torch.isfinite(x[[1, 3]]).all()
    t1 = float(((0.0 - v[0]) / (v[1] - v[0])).detach())
    assert t1 > 1.0 and torch.equal(x[1], (p[0] + t1 * (p[1] - p[0])).detach())     # beyond b: extrapolated
    x.sum().backward()
    assert torch.isfinite(p.grad).all() and torch.isfinite(v.grad).all()
    assert p.grad[[2, 3, 4]].abs().sum() == 0 and v.grad[[2, 3, 4]].abs().sum() == 0
    assert p.grad[[0, 1, 5, 9]].abs().sum() > 0
    gp, gv = radfoam.isosurface_vertices_grad(p.detach(), v.detach(), sites[:1], 0.0, torch.ones(1, 3, dtype=F64))
    assert gp.abs().sum() == 0 and gv.abs().sum() == 0
    bad = torch.ones(4, 3, dtype=F64)
    bad[1, 0] = float("inf")                                                        # an upstream that is not finite
    gp, gv = radfoam.isosurface_vertices_grad(p.detach(), v.detach(), sites, 0.0, bad)
    assert torch.isfinite(gp).all() and torch.isfinite(gv).all() and gp[[0, 1]].abs().sum() == 0 and gp[5].abs().sum() > 0


@pytest.mark.parametrize("n,seed", CLOUDS)
def test_host_build_is_the_torch_backend_bit_for_bit(n, seed):
    import importlib

    import radfoam

    I = importlib.import_module("radfoam_amd.isosurface")      # the package attribute of that name is the function
    c = HI.cloud(n, seed)
    got, host = _np(_torch_mesh(c)), HI.mesh(c["points"], c["tets"], c["values"], 0.0)
    for key in ("vertex_sites", "triangles", "triangle_tet"):
        assert np.array_equal(got[key], host[key]), key
    gap_x, gap_t = np.abs(got["vertices"] - host["vertices"]).max(), np.abs(got["vertex_t"] - host["vertex_t"]).max()
    pts, val, sites = torch.from_numpy(c["points"]), torch.from_numpy(c["values"]), torch.from_numpy(got["vertex_sites"])
    g = torch.randn((len(sites), 3), dtype=F64, generator=torch.Generator().manual_seed(seed))
    parts = I._grad_parts_torch(pts, val, sites, 0.0, g).numpy()
    host_parts = HI.vertices_grad(c["points"], c["values"], got["vertex_sites"], 0.0, g.numpy())
    gap_g = np.abs(parts - host_parts).max()
    print(f"({n}, {seed}): host build against torch: vertices {gap_x:.3g}, t {gap_t:.3g}, backward parts {gap_g:.3g}")
    assert gap_x == 0 and gap_t == 0 and gap_g == 0
    gp, gv = radfoam.isosurface_vertices_grad(pts, val, sites, 0.0, g, backend="torch")
    want = np.zeros((n, 4))
    np.add.at(want, got["vertex_sites"].reshape(-1), host_parts.reshape(-1, 4))
    scale = np.maximum(1.0, np.abs(want).max(1))
    assert (np.abs(np.concatenate([gp.numpy(), gv.numpy()[:, None]], 1) - want).max(1) / scale).max() <= 1e-14
    # the host build counts what it emits and reports an index out of range
    counts, keys, tri_tet, bad = HI.extract(c["points"], c["tets"], c["values"], 0.0)
    assert bad == -1 and np.array_equal(np.bincount(tri_tet, minlength=len(counts)), counts) and (keys >= 0).all()
    broken = c["tets"].copy()
    broken[5, 1] = n
    assert HI.extract(c["points"], broken, c["values"], 0.0)[3] == 5
