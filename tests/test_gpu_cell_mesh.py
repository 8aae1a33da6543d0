"""The welded surface mesh on the GPU (radfoam.cell_mesh, mesh_vertices, mesh_vertices_grad): the device against the host
build of the same arithmetic (tests/host_harness/clip_mesh_host) on the kernel's seams, the topology, cell_surface, the
float64 torch restatement, autograd, and ten steps of an optimisation through the vertices.

hub64's row 0, ring16's 16-gon and the general clouds stay on the lane-per-face kernel; ring17's 17-gon goes through the
serial one; hub65 and hub200 have rows past 64 entries, which the lane-per-face kernel takes as they are (a lane reads its
row from memory).  tests/test_cell_mesh.py holds the host build to scipy's Delaunay tetrahedra and the exact circumcentres.

Measured on the MI355X: device against the host build 0 on all seven clouds (keys, offsets, indices, slots bit-equal, and so
are the positions); max |vertices[triangles] - cell_surface| uniform400 8.6e-14 h, hub64 8.7e-15, hub65 7.5e-15, hub200
1.8e-14, ring16 1.4e-14, ring17 4.5e-14, clustered 1.0e-13, grid 4.9e-15 (about a third of the corners bit-equal, 98 % on the
grid); |enclosed volume - exact| at most 3.4e-16 s^3 (ring17); HIP against the torch restatement, of max(1, |row|):
vertices 1.1e-16 / 0 / 1.8e-16 and gradient 7.9e-16 / 6.6e-16 / 7.4e-16 on uniform400 / hub200 / clustered, against the host
build 0; circumcentres against the clipped vertices 4.4e-14 h; the sphere loss over ten Adam steps 5.83e-3 -> 3.73e-3.
"""
import numpy as np
import pytest
import torch

from tests.host_harness import clip_host as H
from tests.host_harness import clip_mesh_host as HM

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ("uniform400", "hub64", "hub65", "hub200", "ring16", "ring17", "clustered")
EPS = 1e-9
_GPU = {}


def _tensors(c):
    return (torch.from_numpy(c["points"]).to(DEV), torch.from_numpy(c["adjacency"].astype(np.int64)).to(DEV).to(torch.uint32),
            torch.from_numpy(c["offsets"].astype(np.int64)).to(DEV).to(torch.uint32))


def _numpy(mesh):
    return {k: getattr(mesh, k).detach().cpu().numpy() for k in mesh._fields}


def _device_mesh(name):
    """(tensors, inside, CellMesh, the same as numpy) of the named selection, once"""
    if name not in _GPU:
        import radfoam

        t = _tensors(H.case(name))
        inside = torch.from_numpy(HM.selection(name)).to(DEV)
        mesh = radfoam.cell_mesh(*t, inside)
        _GPU[name] = (t, inside, mesh, _numpy(mesh))
    return _GPU[name]


@pytest.mark.parametrize("name", NAMES)
def test_device_agrees_with_the_host_build(name):
    import radfoam

    t, inside, mesh, got = _device_mesh(name)
    want = HM.host_mesh(name)
    assert isinstance(mesh, radfoam.CellMesh) and mesh.vertices.dtype == torch.float64
    for key in mesh._fields[1:]:
        assert getattr(mesh, key).dtype == torch.int64
        assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), key
    diff = np.abs(got["vertices"] - want["vertices"]).max(1) / np.maximum(1.0, np.abs(want["vertices"]).max(1))
    largest = int(np.diff(got["polygon_offsets"]).max())
    print(f"{name}: F {len(got['polygon_slot'])}, C {len(got['polygon_vertices'])}, V {len(got['vertices'])}, largest polygon "
          f"{largest}; max |device - host| / max(1, |row|) = {diff.max():.3g}")
    assert np.isfinite(got["vertices"]).all() and diff.max() <= EPS
    if name in ("ring16", "ring17"):
        assert largest == int(name[4:])                    # on either side of the lane kernel's capacity
    again = _numpy(radfoam.cell_mesh(*t, inside))          # two runs are bit-identical
    for key in mesh._fields:
        assert np.array_equal(again[key], got[key]), key


@pytest.mark.parametrize("name", NAMES)
def test_topology(name):
    got = _device_mesh(name)[3]
    HM.check_topology(got, name)
    HM.check_fans(got)


@pytest.mark.parametrize("name", NAMES + ("grid",))
def test_against_cell_surface(name):
    """the grid (cospherical sites) only here: the geometry is cell_surface's, whatever the keys do"""
    import radfoam

    c = H.case(name)
    t, inside, mesh, got = _device_mesh(name)
    tri, edge = radfoam.cell_surface(*t, inside)
    tri, edge = tri.cpu().numpy(), edge.cpu().numpy()
    assert np.array_equal(got["triangle_slot"], edge)
    mine = got["vertices"][got["triangles"]]
    h = H.GRID_H if name == "grid" else c["h"]
    worst = np.abs(mine - tri).max() / h
    same = (mine == tri).all(2).mean()
    print(f"{name}: max |vertices[triangles] - cell_surface| = {worst:.3g} h; {100.0 * same:.1f} % of the corners bit-equal")
    assert worst <= EPS
    sel = inside.cpu().numpy()
    if name == "grid":
        assert sel.sum() == 64
        H.check_surface(c, sel, mine, edge, 64 * H.GRID_H ** 3, H.GRID_H, counts=False)
    else:
        volume = c["exact"]["volume_f"][sel].sum()
        H.check_surface(c, sel, mine, edge, volume, np.cbrt(volume))


@pytest.mark.parametrize("name", ["uniform400", "hub200", "clustered"])
def test_mesh_vertices_and_their_gradient_against_the_torch_restatement(name):
    import radfoam

    t, inside, mesh, got = _device_mesh(name)
    p, keys = t[0], mesh.vertex_sites
    v = radfoam.mesh_vertices(p, keys)
    ref = radfoam.mesh_vertices(p, keys, backend="torch")
    assert v.dtype == torch.float64 and v.shape == ref.shape == mesh.vertices.shape
    rel = lambda a, b: float(((a - b).abs().amax(1) / b.abs().amax(1).clamp(min=1.0)).max())
    g = torch.from_numpy(np.random.default_rng(4).uniform(-1.0, 1.0, tuple(v.shape))).to(DEV)
    grad = radfoam.mesh_vertices_grad(p, keys, g)
    gref = radfoam.mesh_vertices_grad(p, keys, g, backend="torch")
    host = HM.vertices(H.case(name)["points"], got["vertex_sites"])
    clipped = float(((v - mesh.vertices).abs().amax(1)).max()) / H.case(name)["h"]
    print(f"{name}: HIP against torch: vertices {rel(v, ref):.3g}, gradient {rel(grad, gref):.3g} of max(1, |row|); against "
          f"the host build {np.abs(v.cpu().numpy() - host).max():.3g}; circumcentres against the clipped vertices {clipped:.3g} h")
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0.0
    assert grad.dtype == torch.float64 and grad.shape == (p.shape[0], 3)
    assert rel(v, ref) <= EPS and rel(grad, gref) <= EPS and clipped <= EPS
    assert torch.equal(radfoam.mesh_vertices(p, keys), v)                      # bit-identical across runs
    assert torch.equal(radfoam.mesh_vertices_grad(p, keys, g), grad)
    assert torch.equal(radfoam.mesh_vertices_grad(p, keys, g.float()), radfoam.mesh_vertices_grad(p, keys, g.float().double()))


def test_degenerate_keys_on_the_device():
    import radfoam

    pts = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.25, 0.5, 1.0], [3, 1, 2]], dtype=torch.float32)
    keys = torch.tensor([[0, 1, 2, 3], [0, 1, 2, 4], [0, 1, 1, 4], [0, 1, 2, 6], [-1, 1, 2, 4]], dtype=torch.int64)
    g = torch.ones((5, 3), dtype=torch.float64)
    v = radfoam.mesh_vertices(pts.to(DEV), keys.to(DEV)).cpu()
    assert torch.isnan(v[[0, 2, 3, 4]]).all() and float((v[1] - radfoam.mesh_vertices(pts, keys)[1]).abs().max()) <= 1e-15
    grad = radfoam.mesh_vertices_grad(pts.to(DEV), keys.to(DEV), g.to(DEV)).cpu()
    want = radfoam.mesh_vertices_grad(pts, keys[1:2], g[1:2])
    assert bool(torch.isfinite(grad).all()) and float((grad - want).abs().max()) <= 1e-15 and bool((grad[5] == 0.0).all())
    none = radfoam.mesh_vertices_grad(pts.to(DEV), keys[:0].to(DEV), g[:0].to(DEV))
    assert none.shape == (6, 3) and bool((none == 0.0).all())
    assert radfoam.mesh_vertices(pts.to(DEV), keys[:0].to(DEV)).shape == (0, 3)


def test_autograd_through_the_vertices():
    import radfoam

    t, inside, mesh, got = _device_mesh("hub65")
    assert not mesh.vertices.requires_grad
    points = t[0].clone().requires_grad_(True)
    out = radfoam.cell_mesh(points, t[1], t[2], inside)
    assert out.vertices.requires_grad and torch.equal(out.vertices.detach(), mesh.vertices)      # the clipped values
    for key in mesh._fields[1:]:
        assert not getattr(out, key).requires_grad and torch.equal(getattr(out, key), getattr(mesh, key))
    g = torch.from_numpy(np.random.default_rng(5).uniform(-1.0, 1.0, got["vertices"].shape)).to(DEV)
    (out.vertices * g).sum().backward()
    want = radfoam.mesh_vertices_grad(t[0], mesh.vertex_sites, g)
    assert points.grad.dtype == torch.float32 and float(want.abs().max()) > 0.0
    assert torch.equal(points.grad, want.to(torch.float32))
    again = t[0].clone().requires_grad_(True)                                   # and through mesh_vertices
    (radfoam.mesh_vertices(again, mesh.vertex_sites) * g).sum().backward()
    assert torch.equal(again.grad, points.grad)
    with torch.no_grad():
        assert not radfoam.cell_mesh(points, t[1], t[2], inside).vertices.requires_grad


def _assert_empty(mesh):
    shapes = dict(vertices=(0, 3), vertex_sites=(0, 4), polygon_offsets=(1,), polygon_vertices=(0,), polygon_slot=(0,),
                  triangles=(0, 3), triangle_slot=(0,))
    for key, shape in shapes.items():
        value = getattr(mesh, key)
        assert tuple(value.shape) == shape and value.dtype == (torch.float64 if key == "vertices" else torch.int64)
        assert value.device == torch.device(DEV)
    assert int(mesh.polygon_offsets[0]) == 0


def test_empty_and_invalid_inputs():
    import radfoam

    c = H.case("ring16")
    t, inside, mesh, got = _device_mesh("ring16")
    n = t[0].shape[0]
    _assert_empty(radfoam.cell_mesh(*t, torch.zeros(n, dtype=torch.bool, device=DEV)))            # nothing selected
    _assert_empty(radfoam.cell_mesh(torch.zeros((0, 3), device=DEV), torch.zeros(0, dtype=torch.uint32, device=DEV),
                                    torch.zeros(1, dtype=torch.uint32, device=DEV), torch.zeros(0, dtype=torch.bool, device=DEV)))
    with pytest.raises(ValueError, match="cell_mesh: inside selects an unbounded cell"):
        radfoam.cell_mesh(*t, torch.ones(n, dtype=torch.bool, device=DEV))
    open_cell = int(np.nonzero(c["exact"]["open"])[0][0])
    one = torch.zeros(n, dtype=torch.bool, device=DEV)
    one[open_cell] = True
    with pytest.raises(ValueError, match="unbounded cell"):
        radfoam.cell_mesh(*t, one)
    for bad in (inside.cpu(), inside.to(torch.uint8), inside[:-1]):                               # as cell_surface
        with pytest.raises(RuntimeError, match="inside must be a bool"):
            radfoam.cell_mesh(*t, bad)
        with pytest.raises(RuntimeError, match="inside must be a bool"):
            radfoam.cell_surface(*t, bad)
    with pytest.raises(RuntimeError, match="points must be a float32 CUDA tensor"):
        radfoam.cell_mesh(t[0].double(), t[1], t[2], inside)
    with pytest.raises(RuntimeError, match="expected point_adjacency"):
        radfoam.cell_mesh(t[0], t[1], t[2][:-1], inside)
    adj = c["adjacency"].astype(np.int64)
    adj[int(c["offsets"][40])] = 40          # the site itself in its own row
    with pytest.raises(RuntimeError, match="cell_geometry: cell 40 "):
        radfoam.cell_mesh(t[0], torch.from_numpy(adj).to(DEV), t[2], inside)
    wide = radfoam.cell_mesh(t[0], torch.from_numpy(c["adjacency"].astype(np.int64)).to(DEV),
                             torch.from_numpy(c["offsets"].astype(np.int64)).to(DEV), inside)       # int64 indices
    assert torch.equal(wide.vertices, mesh.vertices) and torch.equal(wide.polygon_vertices, mesh.polygon_vertices)


def test_ten_adam_steps_of_the_sphere_loss_lower_it():
    from examples import foam_mesh

    history = foam_mesh.run(start=H.case("uniform")["points"], steps=10, seed=0, device=DEV, quiet=True)
    print("sphere loss:", " ".join(f"{h[0]:.5g}" for h in history), "vertices:", history[0][1], "->", history[-1][1])
    assert len(history) == 11 and np.isfinite([h[0] for h in history]).all()
    assert history[-1][0] < history[0][0]
