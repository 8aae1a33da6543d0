"""Point gradients of the face areas on the GPU (radfoam.face_area_grad / differentiable_cell_geometry(face_area=True)):
the device operator against the recorded difference quotients of the exact areas (tests/face_area_grad_ref.recorded;
tests/test_face_area_grad.py recomputes them and holds the record to them bit for bit), against the host build of the same
arithmetic (tests/host_harness/clip_area_grad_host) on the kernel's seams, the identities, and autograd.

Device against host: unit upstreams per slot in units of the cells' size (g = r / s, |r| <= 1: every term of a row is
O(1)), bar 1e-9 of max(1, |row|) per row; the two differ only in the order of the sum over a row's faces.  hub64's row 0
and ring16's axis cells stay on the wave-per-cell kernel; hub65's row 0 (65 faces), ring17's axis cells (17-gons) and
redo_spread's four pairs (blocks 0, 0, 1 and 3 of the redo kernel) go through the serial one.

Measured on the MI355X: worst |device - host| / max(1, |row|) hub64 8.7e-16, ring16 7.0e-16, hub65 8.1e-16, ring17 4.3e-16,
redo_spread 1.0e-15; difference quotients, worst |<grad, delta> - R| / spread: uniform400 0.24, hub64 0.12, hub65 0.13,
ring16 0.31, ring17 0.34, redo_spread 0.027; identities on offset 9.1e-16, 7.4e-16, 6.9e-16, on clustered 1.3e-11,
9.8e-13, 2.8e-13 and on the unjittered grid 1.6e-17, 6.3e-18, 1.1e-16 (tests/test_face_area_grad.py says what the grid
asks of the kernel)."""
import numpy as np
import pytest
import torch

from tests import face_area_grad_ref as F
from tests.host_harness import clip_area_grad_host as HA
from tests.host_harness import clip_host as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_GPU = {}


def _tensors(points, offsets, adjacency):
    return (torch.from_numpy(points).to(DEV), torch.from_numpy(adjacency.astype(np.int64)).to(DEV).to(torch.uint32),
            torch.from_numpy(offsets.astype(np.int64)).to(DEV).to(torch.uint32))


def _device_case(key, c):
    """the case's tensors, cell_geometry's answer for them and its face areas as numpy, once"""
    if key not in _GPU:
        import radfoam

        t = _tensors(c["points"], c["offsets"], c["adjacency"])
        geo = radfoam.cell_geometry(*t)
        _GPU[key] = (t, geo, geo.face_area.cpu().numpy())
    return _GPU[key]


def _device_grad(t, geo, g):
    import radfoam

    grad = radfoam.face_area_grad(*t, geo, torch.from_numpy(np.ascontiguousarray(g)).to(DEV))
    assert grad.dtype == torch.float64 and grad.shape == (t[0].shape[0], 3)
    return grad.cpu().numpy()


@pytest.mark.parametrize("name", F.FD_CASES)
def test_device_matches_difference_quotients_of_the_exact_areas(name):
    c, ref = F.case(name), F.recorded(name)
    t, geo, area = _device_case(("rounded", name), c)
    assert np.array_equal(F.kept(c, F.faces_and_weights(c)[0], area), ref["keep"])
    g = np.where(np.isfinite(area), ref["g"], np.nan)          # nothing may read the slots of infinite area
    F.check_against_reference(name, ref, _device_grad(t, geo, g))


@pytest.mark.parametrize("name", ["hub64", "ring16", "hub65", "ring17", "redo_spread"])
def test_device_agrees_with_the_host_build_on_both_paths(name):
    c = F.case(name)
    t, geo, area = _device_case(("rounded", name), c)
    seam = {"hub64": [0], "hub65": [0], "ring16": [0, 1], "ring17": [0, 1],
            "redo_spread": list(np.array(H.REDO_SPREAD_PAIRS).reshape(-1))}[name]
    host_geo = dict(volume=geo.volume.cpu().numpy(), face_area=area)
    assert np.isfinite(host_geo["volume"][seam]).all()
    g = HA.unit_upstream(c, host_geo)               # NaN on the slots of infinite area
    want = HA.face_area_grad(c["points"], c["adjacency"], c["offsets"], area, g)
    assert want["bad"] == 0
    got = _device_grad(t, geo, g)
    diff = np.abs(got - want["grad"]).max(1) / np.maximum(1.0, np.abs(want["grad"]).max(1))
    print(f"{name}: max |device - host| / max(1, |row|) = {diff.max():.3g} over all rows, {diff[seam].max():.3g} on the "
          f"seam rows (max |grad| = {np.abs(want['grad']).max():.3g})")
    assert np.isfinite(got).all() and np.abs(want["grad"][seam]).min() > 0.0 and diff.max() <= 1e-9
    assert np.array_equal(_device_grad(t, geo, g), got)             # two runs are bit-identical


@pytest.mark.parametrize("name", ["offset", "clustered", "grid"])
def test_identities(name):
    c = H.case(name)
    t, geo, area = _device_case(("plain", name), c)
    g = HA.unit_upstream(c, dict(volume=geo.volume.cpu().numpy(), face_area=area))
    HA.check_identities(c["points"], area, g, _device_grad(t, geo, g))


def test_tiny_inputs_give_zeros():
    import radfoam

    tiny = H.tiny_inputs()
    for name in ("n1", "n2", "n4"):              # N <= 4: every face is unbounded, whatever arrives
        t = _tensors(*tiny[name])
        geo = radfoam.cell_geometry(*t)
        e = t[1].shape[0]
        grad = radfoam.face_area_grad(*t, geo, torch.full((e,), float("nan"), dtype=torch.float64, device=DEV))
        assert grad.shape == (t[0].shape[0], 3) and bool((grad == 0.0).all())
    pts = torch.from_numpy(H.case("uniform400")["points"][:50]).to(DEV)          # E = 0
    adj, off = torch.zeros(0, dtype=torch.uint32, device=DEV), torch.zeros(51, dtype=torch.int32, device=DEV)
    geo = radfoam.cell_geometry(pts, adj, off)
    grad = radfoam.face_area_grad(pts, adj, off, geo, torch.zeros(0, device=DEV))
    assert grad.shape == (50, 3) and bool((grad == 0.0).all())
    t = _tensors(*tiny["empty_row"])
    geo = radfoam.cell_geometry(*t)
    off = tiny["empty_row"][1].astype(np.int64)
    c = dict(rows=np.repeat(np.arange(len(off) - 1), np.diff(off)), adjacency=tiny["empty_row"][2])
    g = HA.unit_upstream(c, dict(volume=geo.volume.cpu().numpy(), face_area=geo.face_area.cpu().numpy()))
    grad = _device_grad(t, geo, g)
    assert np.isfinite(grad).all() and (grad[H.EMPTY_ROW_SITE] == 0.0).all() and np.abs(grad).max() > 0.0


def test_differentiable_cell_geometry_with_face_areas():
    import radfoam

    c = F.case("hub65")
    t, geo, _ = _device_case(("rounded", "hub65"), c)
    points = t[0].clone().requires_grad_(True)
    out = radfoam.differentiable_cell_geometry(points, t[1], t[2], face_area=True)
    assert isinstance(out, radfoam.CellGeometry)
    for key in geo._fields:                 # bit-equal to cell_geometry
        assert np.array_equal(getattr(out, key).detach().cpu().numpy(), getattr(geo, key).cpu().numpy(), equal_nan=True)
    assert out.volume.requires_grad and out.centroid.requires_grad and out.face_area.requires_grad
    assert not out.bounded.requires_grad

    target = t[0].double()                  # a constant: the loss depends on points through the geometry alone
    fin = torch.isfinite(geo.face_area)
    b = geo.bounded

    def loss(g, areas=True):
        total = (g.volume[b] ** 2).sum() * 3.0 + ((g.centroid[b] - target[b]) ** 2).sum()
        return total + (g.face_area[fin] ** 2).sum() * 0.5 if areas else total

    loss(out).backward()
    assert points.grad.dtype == torch.float32
    gv = torch.where(b, 6.0 * geo.volume, torch.zeros_like(geo.volume))
    gc = torch.where(b[:, None], 2.0 * (geo.centroid - target), torch.zeros_like(geo.centroid))
    ga = torch.where(fin, geo.face_area, torch.zeros_like(geo.face_area))
    part = radfoam.face_area_grad(*t, geo, ga)
    want = radfoam.cell_geometry_grad(*t, geo, gv, gc) + part
    assert bool(torch.isfinite(want).all()) and float(part.abs().max()) > 0.0
    assert torch.equal(points.grad, want.to(torch.float32))
    # the areas alone: only face_area_grad runs
    alone = t[0].clone().requires_grad_(True)
    (radfoam.differentiable_cell_geometry(alone, t[1], t[2], face_area=True).face_area[fin] ** 2).sum().mul(0.5).backward()
    assert torch.equal(alone.grad, part.to(torch.float32))
    # face_area=False: as before
    plain = t[0].clone().requires_grad_(True)
    out = radfoam.differentiable_cell_geometry(plain, t[1], t[2])
    assert not out.face_area.requires_grad and torch.equal(out.face_area, geo.face_area)
    loss(out, areas=False).backward()
    assert torch.equal(plain.grad, radfoam.cell_geometry_grad(*t, geo, gv, gc).to(torch.float32))


def test_input_validation():
    import radfoam

    c = F.case("ring16")
    t, geo, area = _device_case(("rounded", "ring16"), c)
    e = t[1].shape[0]
    g = torch.ones(e, dtype=torch.float64, device=DEV)
    assert radfoam.face_area_grad(*t, geo, g.float()).dtype == torch.float64            # f32 upstream is accepted
    for bad in (g.cpu(), g.long(), g[:-1], g.reshape(1, -1), None):
        with pytest.raises(RuntimeError, match="grad_face_area must be"):
            radfoam.face_area_grad(*t, geo, bad)
    other = _device_case(("rounded", "ring17"), F.case("ring17"))[1]
    assert other.face_area.shape != geo.face_area.shape
    for bad in (other, geo._replace(face_area=geo.face_area.float()), geo._replace(face_area=geo.face_area.cpu())):
        with pytest.raises(RuntimeError, match="geometry must be the CellGeometry"):
            radfoam.face_area_grad(*t, bad, g)
    with pytest.raises(RuntimeError, match="points must be a float32 CUDA tensor"):
        radfoam.face_area_grad(t[0].double(), t[1], t[2], geo, g)
    adj = c["adjacency"].astype(np.int64)
    adj[int(c["offsets"][40])] = 40          # the site itself in its own row
    with pytest.raises(RuntimeError, match="face_area_grad: cell 40 "):
        radfoam.face_area_grad(t[0], torch.from_numpy(adj).to(DEV), t[2], geo, g)


def test_ten_adam_steps_of_the_surface_loss_lower_it():
    from examples import foam_surface_area

    history = foam_surface_area.run(num_points=2000, steps=10, seed=0, device=DEV, quiet=True)
    print("surface loss:", " ".join(f"{h[0]:.5g}" for h in history), "surface:", f"{history[0][1]:.5g} -> {history[-1][1]:.5g}")
    assert len(history) == 11 and np.isfinite(history).all()
    assert history[-1][0] < history[0][0] and history[-1][1] < history[0][1]
