"""The welded surface mesh, the part that runs without a GPU: radfoam_amd/csrc/rf_clip_mesh.hpp compiled for the host
(tests/host_harness/clip_mesh_host) -- the corner keys against scipy's Delaunay tetrahedra, the welded mesh's topology,
the circumcentre of every key against the clipped corner and against the exact circumcentre of tests/cell_geometry_ref.py
-- and the float64 torch restatement of mesh_vertices / mesh_vertices_grad against its own difference quotients and the
translation, rotation and scaling identities.  tests/test_gpu_cell_mesh.py holds the device to the host build.

The difference quotients of the gradient test are taken of the closed form in exact rational arithmetic
(cell_geometry_ref._circumcentre), not of the float64 forward: at a step of 2^-20 cell sizes a float64 quotient carries
rounding of the order of 1e-16 |L| / h, a thousand to a million times its truncation error, so that R and the spread
formed from it measure that rounding and not the step (its own miss was 1.6 spreads on uniform400 and 283 on hub65; the
test prints it).  The float64 forward is held to the exact circumcentres separately.

Measured on the host, worst over the seven selections of clip_mesh_host.TABLE, in units of the face's diameter:
|circumcentre of the key (double) - clipped corner| 5.0e-12 (uniform), |circumcentre - exact| 2.1e-12 (uniform400),
|clipped corner - exact| 5.0e-12 (uniform); max |vertices[triangles] - cell_surface| 1.0e-13 h (clustered).  Difference
quotients: worst |<grad, delta> - R| / spread 7.9e-5 (uniform400), 1.3e-4 (hub65); identities 1.1e-16, 2.4e-17, 1.7e-17
of sum |p||grad| (uniform400) and 9.3e-17, 4.8e-18, 0 (clustered); host build against torch 1.8e-16 (vertices) and
4.0e-16 (gradient) of max(1, |row|).  The unjittered grid has 574 keys for its 99 distinct corner positions."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import cell_geometry_ref as X
from tests.host_harness import clip_host as H
from tests.host_harness import clip_mesh_host as HM

NAMES = tuple(HM.TABLE)
EPS = 1e-9          # the project's geometry eps


def exact_circumcentre(points, key):
    """f64[3] from cell_geometry_ref's rational circumcentre of the four fp32 sites; None if they are coplanar"""
    fr = [[Fraction(float(x)) for x in points[int(s)]] for s in key]
    scale = max(f.denominator for row in fr for f in row)
    got = X._circumcentre(*(tuple(int(f * scale) for f in row) for row in fr))
    if got is None:
        return None
    num, den = got
    return np.array([float(Fraction(n, den * scale)) for n in num])


def _diameters(mesh):
    """per corner: the largest distance between two corners of its polygon"""
    off, xyz = mesh["polygon_offsets"], mesh["corner_xyz"]
    out = np.empty(len(xyz))
    for f in range(len(off) - 1):
        v = xyz[off[f]:off[f + 1]]
        out[off[f]:off[f + 1]] = np.linalg.norm(v[:, None] - v[None], axis=2).max()
    return out


def test_sources_are_built_but_not_part_of_the_source_hash():
    from radfoam_amd import _lib, build

    names = lambda paths: {os.path.basename(p) for p in paths}
    assert "rf_cell_mesh.hip" in names(build.EXTRA_SOURCES)
    assert {"rf_clip_mesh.hpp", "radfoam_hip_mesh.h"} <= names(build.EXTRA_HEADERS)
    assert not names(build.SOURCES + build.HEADERS) & names(build.EXTRA_SOURCES + build.EXTRA_HEADERS)
    lib = _lib.load()
    for name in ("rf_cell_mesh_emit", "rf_cell_mesh_emit_workspace_bytes", "rf_mesh_vertices", "rf_mesh_vertices_grad"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.rf_cell_mesh_emit_workspace_bytes(1000) >= 1000
    none = [None] * 3
    assert lib.rf_cell_mesh_emit(None, 0, None, None, 0, None, *none, 0, 0, *none, None, 0, None) == 0   # nothing to do
    assert lib.rf_cell_mesh_emit(None, 5, None, None, 0, None, *none, 4, 0, *none, None, 0, None) == -1
    assert "null pointer" in _lib.last_error()
    dummy = np.zeros(64).ctypes.data
    assert lib.rf_cell_mesh_emit(dummy, 5, dummy, dummy, 4, dummy, *([dummy] * 3), 400, 4, *([dummy] * 3), dummy, 2, None) == -2
    assert "workspace" in _lib.last_error()
    assert lib.rf_mesh_vertices(None, 0, None, 0, None, None) == 0
    assert lib.rf_mesh_vertices(None, 5, None, 3, None, None) == -1
    assert lib.rf_mesh_vertices_grad(None, 0, None, 0, None, None, None, None, None, None) == 0
    assert lib.rf_mesh_vertices_grad(None, 5, None, 3, None, None, None, None, None, None) == -1


def test_public_names_and_input_checks_without_a_device():
    import radfoam
    import radfoam_amd

    for name in ("CellMesh", "cell_mesh", "mesh_vertices", "mesh_vertices_grad"):
        assert name in radfoam.__all__ and name in radfoam_amd.__all__ and hasattr(radfoam, name)
    assert radfoam.CellMesh._fields == ("vertices", "vertex_sites", "polygon_offsets", "polygon_vertices", "polygon_slot",
                                        "triangles", "triangle_slot")
    pts = torch.zeros(10, 3)
    adj, off = torch.zeros(5, dtype=torch.uint32), torch.zeros(11, dtype=torch.uint32)
    with pytest.raises(RuntimeError, match="points must be a float32 CUDA tensor"):       # no CPU path, like cell_surface
        radfoam.cell_mesh(pts, adj, off, torch.zeros(10, dtype=torch.bool))
    keys = torch.zeros((2, 4), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="float32 CUDA points"):
        radfoam.mesh_vertices(pts, keys, backend="hip")
    with pytest.raises(ValueError, match="backend must be"):
        radfoam.mesh_vertices(pts, keys, backend="triton")
    for bad in (keys.int(), keys[:, :3], keys.reshape(-1)):
        with pytest.raises(RuntimeError, match="vertex_sites must be"):
            radfoam.mesh_vertices(pts, bad)
    for bad in (torch.zeros(2, 3, dtype=torch.int64), torch.zeros(3, 3), None):
        with pytest.raises(RuntimeError, match="grad_vertices must be"):
            radfoam.mesh_vertices_grad(pts, keys, bad)
    assert radfoam.mesh_vertices(pts, keys[:0]).shape == (0, 3)
    assert radfoam.mesh_vertices_grad(pts, keys[:0], torch.zeros(0, 3)).shape == (10, 3)


@pytest.mark.parametrize("name", NAMES)
def test_corner_keys_are_delaunay_tetrahedra_and_the_counts_are_the_references(name):
    from scipy.spatial import Delaunay

    c, mesh = H.case(name), HM.host_mesh(name)
    tets = {tuple(sorted(t)) for t in Delaunay(c["points"].astype(np.float64)).simplices.tolist()}
    keys = mesh["vertex_sites"]
    assert (np.diff(keys, axis=1) > 0).all()                                      # four distinct sites, ascending
    missing = [tuple(k) for k in keys.tolist() if tuple(k) not in tets]
    assert not missing, f"{len(missing)} of {len(keys)} keys are no tetrahedron of the triangulation: {missing[:3]}"
    order = np.lexsort(keys.T[::-1])
    assert np.array_equal(order, np.arange(len(keys)))                            # rows in ascending lexicographic order
    counts = np.diff(mesh["polygon_offsets"])
    if "slots" in c:
        want = c["slots"]["vertices"][mesh["polygon_slot"]]
    else:                                                                         # 'uniform' carries Qhull's ridges
        rows, adj = c["rows"], c["adjacency"].astype(np.int64)
        want = np.array([c["ref"]["ridge_vertices"][(int(rows[e]), int(adj[e]))] for e in mesh["polygon_slot"]])
    assert np.array_equal(counts, want)
    got = (len(counts), int(counts.sum()), len(keys), int(counts.max()))
    print(f"{name}: {int(mesh['inside'].sum())} cells, F C V largest = {got}")
    assert got == HM.TABLE[name]
    # every corner's key names the face's own two sites
    rows, adj = c["rows"], c["adjacency"].astype(np.int64)
    slot = np.repeat(mesh["polygon_slot"], counts)
    assert ((mesh["corner_sites"] == rows[slot][:, None]).any(1) & (mesh["corner_sites"] == adj[slot][:, None]).any(1)).all()


@pytest.mark.parametrize("name", NAMES)
def test_welded_mesh_is_closed_oriented_and_cell_surfaces_geometry(name):
    c, mesh = H.case(name), HM.host_mesh(name)
    HM.check_topology(mesh, name)
    HM.check_fans(mesh)
    tri, edge = H.host_surface(c, mesh["inside"])
    assert np.array_equal(mesh["triangle_slot"], edge)
    got = mesh["vertices"][mesh["triangles"]]
    own = mesh["corner_xyz"][_own_corners(mesh)]
    assert np.array_equal(own, tri)                    # the corners themselves are cell_surface's, bit for bit
    worst = np.abs(got - tri).max() / c["h"]
    print(f"{name}: max |vertices[triangles] - cell_surface| = {worst:.3g} h")
    assert worst <= EPS


def _own_corners(mesh):
    """[T,3]: the corner indices (v0, vk, vk+1) of every fan triangle"""
    off, out = mesh["polygon_offsets"], []
    for f in range(len(off) - 1):
        for k in range(1, off[f + 1] - off[f] - 1):
            out.append((off[f], off[f] + k, off[f] + k + 1))
    return np.array(out, dtype=np.int64).reshape(-1, 3)


@pytest.mark.parametrize("name", NAMES)
def test_circumcentre_of_every_key_is_the_clipped_corner_and_the_exact_one(name):
    c, mesh = H.case(name), HM.host_mesh(name)
    centre = HM.vertices(c["points"], mesh["vertex_sites"])
    assert np.isfinite(centre).all()
    size = _diameters(mesh)
    pv = mesh["polygon_vertices"]
    clipped = (np.abs(centre[pv] - mesh["corner_xyz"]).max(1) / size).max()        # every corner, not the picked one alone
    exact = np.array([exact_circumcentre(c["points"], k) for k in mesh["vertex_sites"]])
    size_v = np.full(len(centre), np.inf)
    np.minimum.at(size_v, pv, size)                                                # the smallest face around the vertex
    to_exact = (np.abs(centre - exact).max(1) / size_v).max()
    corner_exact = (np.abs(exact[pv] - mesh["corner_xyz"]).max(1) / size).max()
    print(f"{name}: of the face's diameter: |circumcentre - clipped| = {clipped:.3g}, |circumcentre - exact| = "
          f"{to_exact:.3g}, |clipped - exact| = {corner_exact:.3g} (bar {EPS:.3g})")
    assert clipped <= EPS and to_exact <= EPS and corner_exact <= EPS


def test_serial_face_reports_what_it_cannot_write():
    c = H.case("ring17")
    slot = H.slot_of(c, 0, 1)                                                       # the 17-gon between the axis sites
    args = (c["points"], c["adjacency"], c["offsets"], 0, slot)
    assert HM.face_count(*args) == 17 and HM.face_count(*args, cap=16) == -1
    status, xyz, sites = HM.face_corners(*args, 17, cap=17)
    assert status == 0 and np.isfinite(xyz).all() and (sites != HM.NO_SITE).all()
    for expect, cap, want in ((17, 16, 1), (16, 256, 3), (18, 256, 3)):             # too many vertices; another count
        status, xyz, sites = HM.face_corners(*args, expect, cap=cap)
        assert status == want and np.isnan(xyz).all() and (sites == HM.NO_SITE).all()   # void, never stale
    status, xyz, sites = HM.face_corners(c["points"], c["adjacency"], c["offsets"], 1, slot, 17)   # not a's slot
    assert status == 2 and np.isnan(xyz).all()


def test_grid_keeps_cell_surfaces_geometry_without_a_topology_claim():
    c, mesh = H.case("grid"), HM.host_mesh("grid")
    tri, edge = H.host_surface(c, mesh["inside"])
    assert np.array_equal(mesh["triangle_slot"], edge)
    got = mesh["vertices"][mesh["triangles"]]
    worst = np.abs(got - tri).max() / H.GRID_H
    print(f"grid: max |vertices[triangles] - cell_surface| = {worst:.3g} h; {len(mesh['vertices'])} keys for the "
          f"{len(np.unique(np.round(mesh['vertices'] / H.GRID_H * 2), axis=0))} distinct positions")
    assert worst <= EPS
    H.check_surface(c, mesh["inside"], got, mesh["triangle_slot"], 64 * H.GRID_H ** 3, H.GRID_H, counts=False)


# ---- the torch restatement ---------------------------------------------------------------------------------------------

def _probe(name, seed):
    c, mesh = H.case(name), HM.host_mesh(name)
    rng = np.random.default_rng(seed)
    keys = torch.from_numpy(mesh["vertex_sites"])
    g = torch.from_numpy(rng.uniform(-1.0, 1.0, mesh["vertices"].shape))
    return c, mesh, keys, g, rng


@pytest.mark.parametrize("name", ["uniform400", "hub65"])
def test_torch_gradient_matches_its_difference_quotients(name):
    import radfoam

    c, mesh, keys, g, rng = _probe(name, 1)
    p = torch.from_numpy(c["points"]).double()
    h = 2.0 ** -20 * 2.0 ** round(np.log2(c["h"]))            # 2^-20 cell sizes, a power of two: p +- h delta is exact
    loss = lambda q: float((radfoam.mesh_vertices(q, keys, backend="torch") * g).sum())
    q = p.clone().requires_grad_(True)
    out = radfoam.mesh_vertices(q, keys)                      # CPU tensors: the torch restatement
    assert out.dtype == torch.float64 and np.abs(out.detach().numpy() - mesh["vertices"]).max() <= EPS * c["h"]
    (out * g).sum().backward()
    grad = radfoam.mesh_vertices_grad(p, keys, g, backend="torch")
    assert q.grad.dtype == torch.float64 and torch.equal(q.grad, grad)
    touched = np.unique(mesh["vertex_sites"])
    gF = [[Fraction(float(x)) for x in row] for row in g.numpy()]
    worst, noise = 0.0, 0.0
    for _ in range(6):
        delta = torch.zeros_like(p)
        delta[touched] = torch.from_numpy(rng.integers(-8, 9, (len(touched), 3)).astype(np.float64) / 8.0)
        moved = lambda s: (p + s * delta).numpy()               # exact: a dyadic step on dyadic points
        D = lambda s: (_exact_loss(moved(s), mesh["vertex_sites"], gF) - _exact_loss(moved(-s), mesh["vertex_sites"], gF)) / Fraction(2.0 * s)
        d1, d2 = D(h), D(0.5 * h)
        R, spread = float((4 * d2 - d1) / 3), float(abs(d2 - d1))
        got = float((grad * delta).sum())
        d64 = (loss(p + h * delta) - loss(p - h * delta)) / (2.0 * h)
        print(f"{name}: <grad, delta> = {got:+.12e}, R = {R:+.12e}, |difference| = {abs(got - R):.3g}, spread = {spread:.3g}; "
              f"the float64 quotient at h is off R by {abs(d64 - R):.3g}")
        worst, noise = max(worst, abs(got - R) / spread), max(noise, abs(d64 - R) / spread)
        assert abs(got - R) <= spread
    print(f"{name}: worst |<grad, delta> - R| / spread = {worst:.3g} (the float64 quotient's: {noise:.3g})")


def _exact_loss(points64, keys, gF):
    """sum_v g_v . c_v as a Fraction, c_v the rational circumcentre of the key's sites (float64 coordinates taken exactly)"""
    total = Fraction(0)
    cache = {}
    coords = lambda s: cache.setdefault(s, [Fraction(float(x)) for x in points64[s]])
    for key, g in zip(keys.tolist(), gF):
        fr = [coords(s) for s in key]
        scale = max(f.denominator for row in fr for f in row)
        num, den = X._circumcentre(*(tuple(int(f * scale) for f in row) for row in fr))
        total += sum(gk * Fraction(n, den * scale) for gk, n in zip(g, num))
    return total


@pytest.mark.parametrize("name", ["uniform400", "clustered"])
def test_torch_gradient_meets_its_identities(name):
    import radfoam

    c, mesh, keys, g, _ = _probe(name, 2)
    pts = torch.from_numpy(c["points"])
    grad = radfoam.mesh_vertices_grad(pts, keys, g).numpy()                  # float32 CPU points: widened
    centre = radfoam.mesh_vertices(pts, keys).numpy()
    check_identities(c["points"], centre, g.numpy(), grad)


def check_identities(points, centre, g, grad, eps=EPS):
    """sum grad = sum g (a translation moves every vertex along), sum p x grad = sum c x g (a rotation turns them) and
    sum p . grad = sum g . c (a vertex is homogeneous of degree 1), to eps sum |p||grad| (the first times max |p|)"""
    p = points.astype(np.float64)
    assert np.isfinite(grad).all() and np.isfinite(centre).all()
    scale = (np.linalg.norm(p, axis=1) * np.linalg.norm(grad, axis=1)).sum()
    shift = np.abs(grad.sum(0) - g.sum(0)).max() * np.linalg.norm(p, axis=1).max()
    turn = np.abs(np.cross(p, grad).sum(0) - np.cross(centre, g).sum(0)).max()
    euler = abs((p * grad).sum() - (g * centre).sum())
    print(f"identities: |sum grad - sum g| max|p| = {shift / scale:.3g}, |sum p x grad - sum c x g| = {turn / scale:.3g}, "
          f"|sum p.grad - sum g.c| = {euler / scale:.3g}, all of sum |p||grad| = {scale:.4g}")
    assert scale > 0.0 and shift <= eps * scale and turn <= eps * scale and euler <= eps * scale


def test_coplanar_and_invalid_keys_give_nan_forward_and_nothing_backward():
    import radfoam

    pts = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.25, 0.5, 1.0], [3, 1, 2]], dtype=torch.float32)
    keys = torch.tensor([[0, 1, 2, 3],          # coplanar exactly
                         [0, 1, 2, 4],          # a tetrahedron
                         [0, 1, 1, 4],          # a repeated site
                         [0, 1, 2, 6],          # a site out of range
                         [-1, 1, 2, 4]], dtype=torch.int64)
    g = torch.ones((5, 3), dtype=torch.float64)
    v = radfoam.mesh_vertices(pts, keys)
    assert torch.isnan(v[[0, 2, 3, 4]]).all() and torch.isfinite(v[1]).all()
    want = torch.from_numpy(exact_circumcentre(pts.numpy(), [0, 1, 2, 4]))
    assert (v[1] - want).abs().max() <= 1e-15
    grad = radfoam.mesh_vertices_grad(pts, keys, g)
    alone = radfoam.mesh_vertices_grad(pts, keys[1:2], g[1:2])
    assert torch.equal(grad, alone) and bool((grad[[3, 5]] == 0.0).all()) and float(grad.abs().max()) > 0.0
    host = HM.vertices(pts.numpy(), keys.numpy())
    assert np.array_equal(np.isnan(host), np.isnan(v.numpy())) and np.abs(host[1] - v[1].numpy()).max() <= 1e-15
    parts = HM.vertices_grad(pts.numpy(), keys.numpy(), g.numpy())
    assert (parts[[0, 2, 3, 4]] == 0.0).all() and np.abs(parts[1].sum(0) - 1.0).max() <= 1e-15
    q = pts.clone().requires_grad_(True)                    # autograd: float32 in, float32 back
    radfoam.mesh_vertices(q, keys)[1].sum().backward()
    assert q.grad.dtype == torch.float32 and torch.equal(q.grad, alone.float())


@pytest.mark.parametrize("name", ["hub65", "clustered"])
def test_host_build_agrees_with_the_torch_restatement(name):
    import radfoam

    c, mesh, keys, g, _ = _probe(name, 3)
    pts = torch.from_numpy(c["points"])
    v = radfoam.mesh_vertices(pts, keys).numpy()
    host = HM.vertices(c["points"], mesh["vertex_sites"])
    dv = (np.abs(host - v).max(1) / np.maximum(1.0, np.abs(v).max(1))).max()
    parts = HM.vertices_grad(c["points"], mesh["vertex_sites"], g.numpy())
    grad = np.zeros((len(c["points"]), 3))
    np.add.at(grad, mesh["vertex_sites"].reshape(-1), parts.reshape(-1, 3))
    want = radfoam.mesh_vertices_grad(pts, keys, g).numpy()
    dg = (np.abs(grad - want).max(1) / np.maximum(1.0, np.abs(want).max(1))).max()
    print(f"{name}: host against torch: vertices {dv:.3g}, gradient {dg:.3g} of max(1, |row|)")
    assert dv <= EPS and dg <= EPS
