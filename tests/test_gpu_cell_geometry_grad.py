"""Point gradients of the cell geometry on the GPU (radfoam.cell_geometry_grad / differentiable_cell_geometry): the device
operator against the host build of the same arithmetic (tests/host_harness/clip_grad_host) on the kernel's seams, against
the recorded difference quotients of the exact geometry (tests/cell_geometry_grad_ref.recorded; tests/
test_cell_geometry_grad.py recomputes them and holds the record to them bit for bit), the identities, and autograd.

Device against host: unit upstreams per cell in units of the cell's own size (gV = r / s^2, gC = r', |r| <= 1: every row
of the gradient is O(1)), bar 1e-9 per row; the two differ only in the order of the sum over a row's faces.
Measured on the MI355X: worst |device - host| over all rows hub64 7.1e-15, ring16 1.8e-15, hub65 3.6e-15, ring17 6.9e-18,
redo_spread 2.8e-14 (on the seam rows at most 3.6e-15); difference quotients, worst |<grad, delta> - R| / spread:
uniform400 2.8e-6, hub65 3.6e-3; identities on uniform 1.3e-16 and 1.7e-16."""
import numpy as np
import pytest
import torch

from tests import cell_geometry_grad_ref as G
from tests.host_harness import clip_grad_host as HG
from tests.host_harness import clip_host as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_GPU = {}


def _tensors(points, offsets, adjacency):
    return (torch.from_numpy(points).to(DEV), torch.from_numpy(adjacency.astype(np.int64)).to(DEV).to(torch.uint32),
            torch.from_numpy(offsets.astype(np.int64)).to(DEV).to(torch.uint32))


def _device_case(key, c):
    """the case's tensors and cell_geometry's answer for them, once"""
    if key not in _GPU:
        import radfoam

        t = _tensors(c["points"], c["offsets"], c["adjacency"])
        _GPU[key] = (t, radfoam.cell_geometry(*t))
    return _GPU[key]


def _device_grad(t, geo, gv, gc):
    import radfoam

    up = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    grad = radfoam.cell_geometry_grad(*t, geo, up(gv), up(gc))
    assert grad.dtype == torch.float64 and grad.shape == (t[0].shape[0], 3)
    return grad.cpu().numpy()


@pytest.mark.parametrize("name", ["hub64", "ring16", "hub65", "ring17", "redo_spread"])
def test_device_agrees_with_the_host_build_on_both_paths(name):
    """hub64's row 0 and ring16's axis cells stay on the wave-per-cell kernel; hub65's row 0, ring17's axis cells and
    redo_spread's four pairs (blocks 0, 0, 1 and 3 of the redo kernel) go through the serial one."""
    c = G.case(name)
    host = HG.host_forward(("rounded", name), c)
    t, geo = _device_case(("rounded", name), c)
    assert np.array_equal(geo.bounded.cpu().numpy(), host["bounded"])
    seam = {"hub64": [0], "hub65": [0], "ring16": [0, 1], "ring17": [0, 1],
            "redo_spread": list(np.array(H.REDO_SPREAD_PAIRS).reshape(-1))}[name]
    assert host["bounded"][seam].all()
    gv, gc = HG.unit_upstreams(host)
    want = HG.cell_geometry_grad(c["points"], c["adjacency"], c["offsets"], host, gv, gc)
    assert want["bad"] == 0
    got = _device_grad(t, geo, gv, gc)
    diff = np.abs(got - want["grad"]).max(1)
    print(f"{name}: max |device - host| = {diff.max():.3g} over all rows, {diff[seam].max():.3g} on the seam rows "
          f"(max |grad| = {np.abs(want['grad']).max():.3g})")
    assert np.isfinite(got).all() and diff.max() <= 1e-9
    for one in ((gv, None), (None, gc)):
        part = HG.cell_geometry_grad(c["points"], c["adjacency"], c["offsets"], host, *one)["grad"]
        assert np.abs(_device_grad(t, geo, *one) - part).max() <= 1e-9


@pytest.mark.parametrize("name", ["uniform400", "hub65"])
def test_device_matches_difference_quotients_of_the_exact_geometry(name):
    c, ref = G.case(name), G.recorded(name)
    t, geo = _device_case(("rounded", name), c)
    assert np.array_equal(geo.bounded.cpu().numpy(), ref["cells"])
    G.check_against_reference(name, ref, _device_grad(t, geo, ref["w"], ref["u"]))


def test_identities_on_the_uniform_cloud():
    c = H.case("uniform")
    t, geo = _device_case(("plain", "uniform"), c)
    host = dict(volume=geo.volume.cpu().numpy(), centroid=geo.centroid.cpu().numpy(), bounded=geo.bounded.cpu().numpy())
    assert len(c["points"]) == 1500 and host["bounded"].sum() >= 1000
    gv, gc = HG.unit_upstreams(host)
    HG.check_identities(c["points"], host, gv, gc, _device_grad(t, geo, gv, gc))


def test_tiny_inputs_give_finite_numbers():
    import radfoam

    tiny = H.tiny_inputs()
    for name in ("n1", "n2", "n4"):
        t = _tensors(*tiny[name])
        geo = radfoam.cell_geometry(*t)
        n = t[0].shape[0]
        grad = radfoam.cell_geometry_grad(*t, geo, torch.full((n,), float("inf"), dtype=torch.float64, device=DEV),
                                          torch.full((n, 3), float("nan"), dtype=torch.float64, device=DEV))
        assert grad.shape == (n, 3) and bool((grad == 0.0).all())
    t = _tensors(*tiny["empty_row"])
    geo = radfoam.cell_geometry(*t)
    host = dict(volume=geo.volume.cpu().numpy(), bounded=geo.bounded.cpu().numpy())
    gv, gc = HG.unit_upstreams(host)           # NaN on the unbounded cells
    grad = _device_grad(t, geo, gv, gc)
    assert np.isfinite(grad).all() and (grad[H.EMPTY_ROW_SITE] == 0.0).all() and np.abs(grad).max() > 0.0


def test_differentiable_cell_geometry():
    import radfoam

    c = G.case("hub65")
    t, geo = _device_case(("rounded", "hub65"), c)
    points = t[0].clone().requires_grad_(True)
    out = radfoam.differentiable_cell_geometry(points, t[1], t[2])
    assert isinstance(out, radfoam.CellGeometry)
    for key in geo._fields:                 # bit-equal to cell_geometry
        assert np.array_equal(getattr(out, key).detach().cpu().numpy(), getattr(geo, key).cpu().numpy(), equal_nan=True)
    assert out.volume.requires_grad and out.centroid.requires_grad
    assert not out.bounded.requires_grad and not out.face_area.requires_grad

    target = t[0].double()                  # a constant: the loss depends on points through the geometry alone

    def loss(g):
        b = g.bounded
        return (g.volume[b] ** 2).sum() * 3.0 + ((g.centroid[b] - target[b]) ** 2).sum()

    loss(out).backward()
    assert points.grad.dtype == torch.float32
    b = geo.bounded                         # what autograd hands the operator; NaN - x on the unbounded cells is masked
    gv = torch.where(b, 6.0 * geo.volume, torch.zeros_like(geo.volume))
    gc = torch.where(b[:, None], 2.0 * (geo.centroid - target), torch.zeros_like(geo.centroid))
    want = radfoam.cell_geometry_grad(*t, geo, gv, gc)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0.0
    assert torch.equal(points.grad, want.to(torch.float32))
    again = t[0].clone().requires_grad_(True)
    loss(radfoam.differentiable_cell_geometry(again, t[1], t[2])).backward()
    assert torch.equal(again.grad, points.grad)                     # two runs are bit-identical
    # the operator alone, too
    assert torch.equal(radfoam.cell_geometry_grad(*t, geo, gv, None), radfoam.cell_geometry_grad(*t, geo, gv, None))
    adj = c["adjacency"].astype(np.int64)
    adj[int(c["offsets"][40])] = 40          # the site itself in its own row
    bad = torch.from_numpy(adj).to(DEV)
    with pytest.raises(RuntimeError, match="cell 40 "):
        radfoam.differentiable_cell_geometry(points, bad, t[2])
    with pytest.raises(RuntimeError, match="cell_geometry_grad: cell 40 "):
        radfoam.cell_geometry_grad(t[0], bad, t[2], geo, gv, None)


def test_twenty_adam_steps_of_the_lloyd_loss_lower_it():
    from examples import foam_lloyd

    losses = foam_lloyd.run(num_points=2000, steps=20, seed=0, device=DEV, quiet=True)
    print("lloyd loss:", " ".join(f"{x:.5g}" for x in losses))
    assert len(losses) == 21 and np.isfinite(losses).all() and losses[-1] < losses[0]
