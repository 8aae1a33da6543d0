"""Point gradients of the cells' second moments on the GPU (radfoam.cell_moments_grad / differentiable_cell_moments): the
device operator against the recorded difference quotients of the exact moments (tests/cell_moments_grad_ref.recorded;
tests/test_cell_moments_grad.py recomputes probes of every case and holds the record to them bit for bit), against the
host build of the same arithmetic (tests/host_harness/clip_moments_grad_host) on the kernel's seams, the closed form of
the centroidal-Voronoi energy, the identities, and autograd.

hub64's row 0 and ring16's axis cells stay on the wave-per-cell kernel; hub65's row 0, ring17's axis cells and
redo_spread's four pairs (blocks 0, 0, 1 and 3 of the redo kernel) go through the serial one.  The clouds are 365 to 476
points: the smallest at which these seams exist.

Device against host: unit upstreams per cell in units of the cell's own size (r / s^4, |r| <= 1), bar 1e-9 of the row's
scale max(1, max |host row|) per row; the two differ only in the order of the sum over a row's faces.
Measured on the MI355X: difference quotients, worst |<grad, delta> - R| / spread: uniform400 4.7e-7, hub64 4.4e-4,
hub65 2.7e-3, ring16 2.4e-2, ring17 5.8e-3, redo_spread 2.7e-3; worst |device - host| / scale over all rows hub64 2.9e-15,
ring16 7.1e-15, hub65 3.9e-15, ring17 1.4e-17, redo_spread 1.4e-14 (on the seam rows at most 1.4e-15); closed form 4.3e-16
on uniform400's 159 cells and 5.4e-16 on 2,759 cells of the GPU triangulation; identities at most 1.1e-12 (clustered)."""
import numpy as np
import pytest
import torch

from tests import cell_moments_grad_ref as MG
from tests.host_harness import clip_grad_host as HG
from tests.host_harness import clip_host as H
from tests.host_harness import clip_moments_grad_host as HMG

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_GPU = {}


def _tensors(points, offsets, adjacency):
    return (torch.from_numpy(points).to(DEV), torch.from_numpy(adjacency.astype(np.int64)).to(DEV).to(torch.uint32),
            torch.from_numpy(offsets.astype(np.int64)).to(DEV).to(torch.uint32))


def _device_case(key, c):
    """the case's tensors and cell_moments' answer for them, once"""
    if key not in _GPU:
        import radfoam

        t = _tensors(c["points"], c["offsets"], c["adjacency"])
        _GPU[key] = (t, radfoam.cell_moments(*t))
    return _GPU[key]


def _up(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _device_grad(t, geo, gq, gc):
    import radfoam

    grad = radfoam.cell_moments_grad(*t, geo, _up(gq), _up(gc))
    assert grad.dtype == torch.float64 and grad.shape == (t[0].shape[0], 3)
    return grad.cpu().numpy()


def _as_host(mo):
    geo = mo.geometry
    return dict(volume=geo.volume.cpu().numpy(), centroid=geo.centroid.cpu().numpy(), bounded=geo.bounded.cpu().numpy(),
                site=mo.site_moment.cpu().numpy(), central=mo.central_moment.cpu().numpy())


@pytest.mark.parametrize("name", MG.FD_CASES)
def test_device_matches_difference_quotients_of_the_exact_moments(name):
    c, ref = MG.case(name), MG.recorded(name)
    t, mo = _device_case(("rounded", name), c)
    assert np.array_equal(MG.loss_cells(name, mo.geometry.bounded.cpu().numpy()), ref["cells"])
    worst = MG.check_against_reference(name, ref, _device_grad(t, mo.geometry, ref["A"], ref["B"]))
    print(f"{name}: worst |<grad, delta> - R| / spread = {worst:.3g}")


@pytest.mark.parametrize("name", ["hub64", "ring16", "hub65", "ring17", "redo_spread"])
def test_device_agrees_with_the_host_build_on_both_paths(name):
    c = MG.case(name)
    host = HG.host_forward(("rounded", name), c)
    t, mo = _device_case(("rounded", name), c)
    assert np.array_equal(mo.geometry.bounded.cpu().numpy(), host["bounded"])
    seam = {"hub64": [0], "hub65": [0], "ring16": [0, 1], "ring17": [0, 1],
            "redo_spread": list(np.array(H.REDO_SPREAD_PAIRS).reshape(-1))}[name]
    assert host["bounded"][seam].all()
    gq, gc = HMG.unit_upstreams(host)
    for one in ((gq, gc), (gq, None), (None, gc)):                # either upstream None
        want = HMG.cell_moments_grad(c["points"], c["adjacency"], c["offsets"], host, *one)
        assert want["bad"] == 0
        HMG.check_rows_against_host(name, _device_grad(t, mo.geometry, *one), want["grad"], seam)


def test_the_cvt_energy_has_the_classical_gradient_and_the_identities_hold():
    c = H.case("uniform400")
    t, mo = _device_case(("plain", "uniform400"), c)
    fwd = _as_host(mo)
    grad = _device_grad(t, mo.geometry, HMG.trace_upstream(fwd), None)
    assert HMG.check_closed_form(c, fwd, grad) >= 100
    gq, gc = HMG.unit_upstreams(fwd)
    HMG.check_identities(c["points"], fwd, gq, gc, _device_grad(t, mo.geometry, gq, gc))


@pytest.mark.parametrize("name", ["offset", "clustered", "grid"])
def test_identities_far_from_the_origin_on_cells_of_very_different_sizes_and_on_a_grid(name):
    c = H.case(name)
    t, mo = _device_case(("plain", name), c)
    fwd = _as_host(mo)
    gq, gc = HMG.unit_upstreams(fwd)
    HMG.check_identities(c["points"], fwd, gq, gc, _device_grad(t, mo.geometry, gq, gc))


def test_index_dtypes_absent_upstreams_and_repeat_runs_give_the_same_bits():
    import radfoam

    c = MG.case("ring17")
    t, mo = _device_case(("rounded", "ring17"), c)
    geo = mo.geometry
    gq, gc = (_up(x) for x in HMG.unit_upstreams(_as_host(mo)))
    base = radfoam.cell_moments_grad(*t, geo, gq, gc)
    assert bool(torch.isfinite(base).all()) and float(base[:2].abs().max()) > 0.0
    assert torch.equal(radfoam.cell_moments_grad(*t, geo, gq, gc), base)                              # two calls
    for dtype in (torch.int32, torch.int64):                                                          # next to uint32
        assert torch.equal(radfoam.cell_moments_grad(t[0], t[1].to(dtype), t[2].to(dtype), geo, gq, gc), base)
    assert torch.equal(radfoam.cell_moments_grad(*t, geo, gq.float().double(), gc),
                       radfoam.cell_moments_grad(*t, geo, gq.float(), gc))                            # f32 upstreams
    zero = torch.zeros_like(gq)
    assert torch.equal(radfoam.cell_moments_grad(*t, geo, gq), radfoam.cell_moments_grad(*t, geo, gq, zero))
    assert torch.equal(radfoam.cell_moments_grad(*t, geo, None, gc), radfoam.cell_moments_grad(*t, geo, zero, gc))
    assert bool((radfoam.cell_moments_grad(*t, geo) == 0.0).all())
    with pytest.raises(RuntimeError, match="geometry must be the CellGeometry"):
        radfoam.cell_moments_grad(*t, geo._replace(volume=geo.volume.float()), gq, gc)
    with pytest.raises(RuntimeError, match="grad_site_moment must be a floating-point CUDA tensor"):
        radfoam.cell_moments_grad(*t, geo, gq[:, :3], gc)


def test_tiny_inputs_give_finite_numbers():
    import radfoam

    tiny = H.tiny_inputs()
    for name in ("n1", "n2", "n4"):
        t = _tensors(*tiny[name])
        geo = radfoam.cell_geometry(*t)
        n = t[0].shape[0]
        grad = radfoam.cell_moments_grad(*t, geo, torch.full((n, 6), float("inf"), dtype=torch.float64, device=DEV),
                                         torch.full((n, 6), float("nan"), dtype=torch.float64, device=DEV))
        assert grad.shape == (n, 3) and bool((grad == 0.0).all())
    t = _tensors(*tiny["empty_row"])
    geo = radfoam.cell_geometry(*t)
    host = dict(volume=geo.volume.cpu().numpy(), bounded=geo.bounded.cpu().numpy())
    gq, gc = HMG.unit_upstreams(host)           # NaN on the unbounded cells
    grad = _device_grad(t, geo, gq, gc)
    assert np.isfinite(grad).all() and (grad[H.EMPTY_ROW_SITE] == 0.0).all() and np.abs(grad).max() > 0.0


def test_differentiable_cell_moments():
    import radfoam

    c = MG.case("hub65")
    t, mo = _device_case(("rounded", "hub65"), c)
    geo = mo.geometry
    points = t[0].clone().requires_grad_(True)
    out = radfoam.differentiable_cell_moments(points, t[1], t[2])
    assert isinstance(out, radfoam.CellMoments) and isinstance(out.geometry, radfoam.CellGeometry)
    same = lambda x, y: np.array_equal(x.detach().cpu().numpy(), y.cpu().numpy(), equal_nan=True)
    assert same(out.site_moment, mo.site_moment) and same(out.central_moment, mo.central_moment)     # bit-equal
    for key in geo._fields:
        assert same(getattr(out.geometry, key), getattr(geo, key))
    assert out.site_moment.requires_grad and out.central_moment.requires_grad
    assert out.geometry.volume.requires_grad and out.geometry.centroid.requires_grad
    assert not out.geometry.bounded.requires_grad and not out.geometry.face_area.requires_grad

    def loss(m):
        b = m.geometry.bounded
        return m.site_moment[b][:, :3].sum() + (m.central_moment[b][:, :3].sum(1) / m.geometry.volume[b]).sum()

    loss(out).backward()
    assert points.grad.dtype == torch.float32
    # the two operators called by hand with what autograd hands them: the loss's own gradients with respect to the
    # moments and the volume as leaves (zero on the unbounded cells, which the loss masks out)
    b = geo.bounded
    leaves = [x.clone().requires_grad_(True) for x in (mo.site_moment, mo.central_moment, geo.volume)]
    gq, gc, gv = torch.autograd.grad(loss(radfoam.CellMoments(leaves[0], leaves[1], geo._replace(volume=leaves[2]))),
                                     leaves)
    trace = torch.tensor([1.0, 1.0, 1.0, 0.0, 0.0, 0.0], dtype=torch.float64, device=DEV)
    assert torch.equal(gq, b[:, None].double() * trace) and bool((gc[~b] == 0.0).all()) and bool((gv[~b] == 0.0).all())
    assert bool((gc[b][:, :3] > 0.0).all()) and bool((gv[b] < 0.0).all())
    want = radfoam.cell_moments_grad(*t, geo, gq, gc) + radfoam.cell_geometry_grad(*t, geo, gv, None)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0.0
    assert torch.equal(points.grad, want.to(torch.float32))
    again = t[0].clone().requires_grad_(True)
    loss(radfoam.differentiable_cell_moments(again, t[1], t[2])).backward()
    assert torch.equal(again.grad, points.grad)                     # two runs are bit-identical
    # the moments alone: the geometry operator is not needed and the result is cell_moments_grad's
    alone = t[0].clone().requires_grad_(True)
    m = radfoam.differentiable_cell_moments(alone, t[1], t[2])
    m.site_moment[b][:, :3].sum().backward()
    assert torch.equal(alone.grad, radfoam.cell_moments_grad(*t, geo, gq).to(torch.float32))
    # cell_moments itself stays outside autograd
    plain = radfoam.cell_moments(t[0].clone().requires_grad_(True), t[1], t[2])
    assert not plain.site_moment.requires_grad and not plain.central_moment.requires_grad
    adj = c["adjacency"].astype(np.int64)
    adj[int(c["offsets"][40])] = 40          # the site itself in its own row
    bad = torch.from_numpy(adj).to(DEV)
    with pytest.raises(RuntimeError, match="cell 40 "):
        radfoam.differentiable_cell_moments(points, bad, t[2])
    with pytest.raises(RuntimeError, match="cell_moments_grad: cell 40 "):
        radfoam.cell_moments_grad(t[0], bad, t[2], geo, gq, None)


def test_twenty_adam_steps_of_the_cvt_energy_lower_it_and_the_penalty_lowers_the_anisotropy():
    from examples import foam_cvt

    last = {}
    for lam in (0.0, 5.0):
        history = np.array(foam_cvt.run(num_points=2000, steps=20, lam=lam, seed=0, device=DEV, quiet=True))
        print(f"lambda {lam}: loss", " ".join(f"{x:.5g}" for x in history[:, 0]))
        print(f"lambda {lam}: first and last (loss, CVT energy, Lloyd surrogate, anisotropy):", history[0], history[-1])
        assert history.shape == (21, 4) and np.isfinite(history).all() and history[-1, 0] < history[0, 0]
        assert history[-1, 1] < history[0, 1]                 # the energy itself, not only its mean
        assert (history[:, 2] < history[:, 1]).all()          # the surrogate is a part of the energy
        last[lam] = history[-1]
    assert last[5.0][3] < last[0.0][3]                        # the same start, the same steps: the penalty is felt


def test_a_257_gon_raises_naming_an_axis_cell():
    import radfoam
    from radfoam_amd import foam

    pts = H._CLOUDS["ring257"]()
    off, adj = foam.delaunay_csr(pts)
    t = _tensors(pts, off, adj)
    geo = H.cell_geometry(pts, adj, off, cap=512)      # a geometry that had room for the 257-gon (the host build)
    assert geo["bad"] == 0 and geo["bounded"][:2].all()
    roomy = radfoam.CellGeometry(*(torch.from_numpy(np.ascontiguousarray(geo[k])).to(DEV)
                                   for k in ("volume", "centroid", "bounded", "face_area")))
    gq, gc = (_up(x) for x in HMG.unit_upstreams(geo))
    with pytest.raises(RuntimeError, match=r"cell_moments_grad: cell [01] is not supported: a face outgrew 256 vertices"):
        radfoam.cell_moments_grad(*t, roomy, gq, gc)


def test_the_gpu_triangulation_feeds_straight_in():
    """4,000 uniform points, the GPU's own CSR, end to end through autograd: every row finite, the translation identity,
    and the classical gradient of the centroidal-Voronoi energy where it applies."""
    import radfoam
    from radfoam_amd.triangulation import Triangulation

    gen = torch.Generator(device="cpu").manual_seed(0)
    start = (torch.rand((4000, 3), generator=gen) * 2.0 - 1.0).to(DEV)
    tri = Triangulation(start)
    points = start[tri.permutation().to(torch.int64)].contiguous().requires_grad_(True)
    adj, off = tri.point_adjacency(), tri.point_adjacency_offsets()
    mo = radfoam.differentiable_cell_moments(points, adj, off)
    b = mo.geometry.bounded
    assert int(b.sum()) > 3000 and int((~b).sum()) > 0
    mo.site_moment[b][:, :3].sum().backward()
    grad = points.grad.double().cpu().numpy()
    assert np.isfinite(grad).all() and np.abs(grad).max() > 0.0
    c = dict(points=points.detach().cpu().numpy(), offsets=off.to(torch.int64).cpu().numpy(),
             adjacency=adj.to(torch.int64).cpu().numpy())
    fwd = dict(volume=mo.geometry.volume.detach().cpu().numpy(), centroid=mo.geometry.centroid.detach().cpu().numpy(),
               bounded=b.cpu().numpy())
    exact = radfoam.cell_moments_grad(points.detach(), adj, off, mo.geometry, _up(HMG.trace_upstream(fwd))).cpu().numpy()
    assert np.array_equal(exact.astype(np.float32), points.grad.cpu().numpy())
    assert HMG.check_closed_form(c, fwd, exact) > 1500
