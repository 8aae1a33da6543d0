"""Marching tetrahedra on the GPU (radfoam.isosurface, isosurface_vertices, isosurface_vertices_grad): the kernels of
rf_isosurface.hip against the torch backend on the same device and the host build of the same header
(tests/host_harness/iso_host), bit for bit in everything the forward gives; the backward's gather to rounding (the torch
restatement adds a site's incidences in another order); seams of the lane-per-tetrahedron launch; both index widths; the
range check; autograd end to end; the topology of the device's own result.  tests/test_isosurface.py holds the torch
backend and the host build to the table-free reference.

Bounds.  Forward: equality, the operations are spelled and nothing fuses.  isosurface_vertices_grad: 1e-14 of
max(1, |row|), a few dozen float64 roundings of a sum of at most a few dozen incidences.  Autograd end to end returns
float32 (the dtype of the inputs): two float64 results that agree to 1e-14 round to float32 values at most one unit in the
last place apart, 2^-23 of max(1, |row|).

Measured on the MI355X: every forward comparison equal; isosurface_vertices_grad against torch at most 5.3e-16 (points)
and 8.7e-16 (values) of max(1, |row|) over the four clouds, against the host build's parts added in the kernel's order 0;
autograd end to end 0 * 2^-23; the example's sphere loss 1.86e-3 -> 3.46e-4 over 8 steps.  The whole file runs in under 6
s.  Times at 2 M points: DESIGN.md, "Isosurface of an interpolated field"."""
import numpy as np
import pytest
import torch

from tests.host_harness import iso_host as HI

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CLOUDS = tuple(HI.CLOUDS)
F64 = torch.float64
_GPU = {}


def _np(mesh):
    return {k: getattr(mesh, k).detach().cpu().numpy() for k in mesh._fields}


def _device(n, seed):
    """(points, tets int64, values) on the device, the HIP IsoMesh and the same as numpy, once"""
    if (n, seed) not in _GPU:
        import radfoam

        c = HI.cloud(n, seed)
        t = tuple(torch.from_numpy(c[k]).to(DEV) for k in ("points", "tets", "values"))
        mesh = radfoam.isosurface(*t, 0.0)
        _GPU[(n, seed)] = (t, mesh, _np(mesh))
    return _GPU[(n, seed)]


def _same(a, b, label=""):
    for key in a:
        assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key], equal_nan=True), (label, key)


@pytest.mark.parametrize("n,seed", CLOUDS)
def test_kernels_are_the_torch_backend_and_the_host_build_bit_for_bit(n, seed):
    import radfoam

    (pts, tets, val), mesh, got = _device(n, seed)
    nt, nv, nf = HI.CLOUDS[(n, seed)]
    assert isinstance(mesh, radfoam.IsoMesh) and mesh.vertices.is_cuda
    assert got["vertices"].shape == (nv, 3) and got["triangles"].shape == (nf, 3) and np.isfinite(got["vertices"]).all()
    _same(got, _np(radfoam.isosurface(pts, tets, val, 0.0, backend="torch")), "torch")
    c = HI.cloud(n, seed)
    _same(got, HI.mesh(c["points"], c["tets"], c["values"], 0.0), "host build")
    _same(got, _np(radfoam.isosurface(pts, tets, val, 0.0, backend="hip")), "second run")
    for dtype in (torch.uint32, torch.int32):                          # the 16-byte rows; int64 above takes the 32-byte ones
        _same(got, _np(radfoam.isosurface(pts, tets.to(dtype), val, 0.0)), str(dtype))
    again = radfoam.isosurface_vertices(pts, val, mesh.vertex_sites, 0.0)
    assert torch.equal(again, mesh.vertices)                           # the fixed topology gives the mesh's own vertices


@pytest.mark.parametrize("count", (0, 1, 63, 64, 65, 257))
def test_seams_of_the_launch(count):
    import radfoam

    (pts, tets, val), _, _ = _device(400, 1)
    got = _np(radfoam.isosurface(pts, tets[:count], val, 0.0))
    _same(got, _np(radfoam.isosurface(pts, tets[:count], val, 0.0, backend="torch")), count)
    assert (len(got["triangles"]) == 0) == (count < 2)                 # the first tetrahedron alone has no crossing
    if count == 257:
        _same(got, _np(radfoam.isosurface(pts, tets[:count].to(torch.uint32), val, 0.0)), "uint32")
        flat = tets[:count].to(torch.int32).reshape(-1)
        odd = torch.cat([flat[:1], flat])[1:].view(-1, 4)              # rows that start 4 bytes into their storage
        assert odd.data_ptr() % 16 == 4
        _same(got, _np(radfoam.isosurface(pts, odd, val, 0.0)), "a view that is not 16-byte aligned")


def test_all_sixteen_masks_on_both_orientations():
    import radfoam

    level = 0.25
    pts, tets = HI.mask_pair()
    for mask in range(16):
        values = HI.mask_values(mask, level)
        got = _np(radfoam.isosurface(torch.from_numpy(pts).to(DEV), torch.from_numpy(tets).to(DEV),
                                     torch.from_numpy(values).to(DEV), level))
        _same(got, HI.mesh(pts, tets, values, level), mask)
        want = {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[bin(mask).count("1")]
        assert np.array_equal(np.bincount(got["triangle_tet"], minlength=2), [want, want])


def test_index_out_of_range_raises_and_the_next_call_works():
    import radfoam

    (pts, tets, val), _, got = _device(400, 1)
    for dtype, index in ((torch.int64, 400), (torch.int64, -1), (torch.int64, 2 ** 40), (torch.int32, -1), (torch.uint32, 400)):
        broken = tets.clone()
        broken[300, 3] = index
        broken[2000, 0] = 400
        with pytest.raises(RuntimeError, match=r"tetrahedron 300 has a corner index outside \[0, 400\)"):
            radfoam.isosurface(pts, broken.to(dtype), val, 0.0)
        _same(got, _np(radfoam.isosurface(pts, tets.to(dtype), val, 0.0)), "after the error")
    nan = radfoam.isosurface_vertices(pts, val, torch.tensor([[0, 400], [-1, 3]], device=DEV), 0.0)
    assert torch.isnan(nan).all()                                      # sites out of range: NaN, nothing read
    gp, gv = radfoam.isosurface_vertices_grad(pts, val, torch.tensor([[0, 400], [-1, 3]], device=DEV), 0.0,
                                              torch.ones(2, 3, device=DEV))
    assert gp.abs().sum() == 0 and gv.abs().sum() == 0


@pytest.mark.parametrize("n,seed", CLOUDS)
def test_backward_operator_against_torch_and_reproducible(n, seed):
    import radfoam

    (pts, tets, val), mesh, _ = _device(n, seed)
    sites = mesh.vertex_sites
    g = torch.randn((sites.size(0), 3), dtype=F64, generator=torch.Generator().manual_seed(seed)).to(DEV)
    gp, gv = radfoam.isosurface_vertices_grad(pts, val, sites, 0.0, g)
    assert gp.dtype == gv.dtype == F64 and gp.shape == (n, 3) and gv.shape == (n,)
    wp, wv = radfoam.isosurface_vertices_grad(pts, val, sites, 0.0, g, backend="torch")
    for mine, want, label in ((gp, wp, "points"), (gv[:, None], wv[:, None], "values")):
        miss = float(((mine - want).abs().amax(1) / want.abs().amax(1).clamp(min=1.0)).max())
        print(f"({n}, {seed}): isosurface_vertices_grad HIP against torch, {label}: {miss:.3g} of max(1, |row|)")
        assert torch.isfinite(mine).all() and miss <= 1e-14
    # the host build's parts, added in the kernel's order (ascending incidence within a site), give the same bits
    c = HI.cloud(n, seed)
    parts = HI.vertices_grad(c["points"], c["values"], sites.cpu().numpy(), 0.0, g.cpu().numpy()).reshape(-1, 4)
    flat = sites.cpu().numpy().reshape(-1)
    want = np.zeros((n, 4))
    for at in np.argsort(flat, kind="stable"):
        want[flat[at]] += parts[at]
    assert np.array_equal(gp.cpu().numpy(), want[:, :3]) and np.array_equal(gv.cpu().numpy(), want[:, 3])
    ap, av = radfoam.isosurface_vertices_grad(pts, val, sites, 0.0, g)
    assert torch.equal(ap, gp) and torch.equal(av, gv)                 # two runs are bit-identical
    # a stale topology: v_a == v_b is NaN forward and adds nothing backward
    flat_val = val.clone()
    a, b = (int(s) for s in sites[0])
    flat_val[b] = flat_val[a]
    x = radfoam.isosurface_vertices(pts, flat_val, sites, 0.0)
    assert torch.isnan(x[0]).all() and torch.isfinite(x[~((sites == a) | (sites == b)).any(1)]).all()
    sp, sv = radfoam.isosurface_vertices_grad(pts, flat_val, sites[:1], 0.0, g[:1])
    assert sp.abs().sum() == 0 and sv.abs().sum() == 0


def test_autograd_end_to_end():
    import radfoam

    (pts, tets, val), _, _ = _device(400, 1)
    w = torch.randn((HI.CLOUDS[(400, 1)][1], 3), dtype=F64, generator=torch.Generator().manual_seed(9)).to(DEV)
    grads = {}
    for backend in ("hip", "torch"):
        p, v = pts.clone().requires_grad_(True), val.clone().requires_grad_(True)
        mesh = radfoam.isosurface(p, tets, v, 0.0, backend=backend)
        assert mesh.vertices.requires_grad and not mesh.vertex_t.requires_grad
        ((w * torch.sin(1.3 * mesh.vertices)).sum() + 0.5 * (mesh.vertices ** 2).sum()).backward()
        assert p.grad.dtype == torch.float32 and v.grad.dtype == torch.float32
        assert p.grad.abs().sum() > 0 and v.grad.abs().sum() > 0
        grads[backend] = (p.grad, v.grad[:, None])
    for mine, want, label in zip(grads["hip"], grads["torch"], ("points", "values")):
        miss = float(((mine - want).abs().amax(1) / want.abs().amax(1).clamp(min=1.0)).max())
        print(f"autograd through isosurface, HIP against torch, {label}: {miss / 2.0 ** -23:.3g} * 2^-23 of max(1, |row|)")
        assert torch.isfinite(mine).all() and miss <= 2.0 ** -23
    # sum_v x_v moves with its sites: every vertex hands its upstream on in full (float64 sums, rounded once per site)
    p = pts.clone().requires_grad_(True)
    mesh = radfoam.isosurface(p, tets, val, 0.0)
    mesh.vertices.sum().backward()
    total = 3 * mesh.vertices.size(0)
    assert abs(float(p.grad.to(F64).sum()) - total) <= 2.0 ** -24 * float(p.grad.to(F64).abs().sum()) + 1e-12 * total


def test_device_mesh_is_closed_oriented_and_of_genus_zero():
    _, _, got = _device(1000, 3)
    nt, nv, nf = HI.CLOUDS[(1000, 3)]
    assert HI.check_closed(got, "(1000, 3) on the device") == (nv, 3 * nf // 2, nf)
    volume = HI.enclosed_volume(got)
    assert 0.0 < volume < 4.0 / 3.0 * np.pi * HI.RADIUS ** 3
    assert (np.diff(got["triangle_tet"]) >= 0).all()
    sites = got["vertex_sites"]
    assert (np.diff(sites[:, 0] * 2 ** 32 + sites[:, 1]) > 0).all()


def test_example_pulls_the_level_set_onto_a_sphere(tmp_path):
    from examples import foam_isosurface

    ply = tmp_path / "surface.ply"
    history = foam_isosurface.run(num_points=2000, steps=8, every=4, seed=0, device=DEV, quiet=True, ply=str(ply))
    print("sphere loss:", " ".join(f"{h[0]:.5g}" for h in history), "vertices:", history[0][1], "->", history[-1][1])
    assert len(history) == 9 and np.isfinite([h[0] for h in history]).all()
    assert [h[3] for h in history] == [True, False, False, False, True, False, False, False, True]
    assert history[-1][0] < history[0][0]
    head = ply.read_text().split("end_header")[0]
    assert f"element vertex {history[-1][1]}" in head and f"element face {history[-1][2]}" in head and "uchar red" in head
