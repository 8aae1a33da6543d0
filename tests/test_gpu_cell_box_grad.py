"""Point gradients of the cells clipped to a box on the GPU (radfoam.cell_geometry_in_box_grad and
radfoam.differentiable_cell_geometry_in_box, the kernels of rf_cell_box_grad.hip) through the checks of
tests/test_cell_box_grad.py (tests/host_harness/clip_box_grad_host): the recorded difference quotients of the exact
rational boxed geometry (tests/golden/cell_box_grad/fd.npz; the rational code is not run here), the identities of a
partition of a fixed box, agreement with cell_geometry_grad away from the walls and with the host build row by row, the
seams between the lane-per-face kernel and the serial one, refusals, input forms, autograd and the example.

Rows of up to 64 faces (lists of up to 70 planes) whose row polygons stay within 16 vertices are on the wave-per-cell
kernel: hub58, hub59 and hub64's site 0 and ring16_cut's axis sites.  hub65's site 0 (65 faces), ring17_cut's axis
sites and redo_spread_cut's eight (blocks 0, 1 and 3 of the redo kernel) go through the serial one.

Measured on the MI355X, worst |<grad, delta> - R| / spread: uniform400 1.4e-5, tight 1.2e-4, hub58 1.7e-2, hub59 0.63,
hub64 9.7e-3, hub65 5.9e-3, ring16_cut 1.4e-3, ring17_cut 4.0e-3, redo_spread_cut 1.0e-2; the first-moment partition at
most 1.8e-16 (wide) of the grad_centroid half; against cell_geometry_grad on wide 1.2e-12; device against host build per
row at most 7.4e-15; the GPU triangulation of 20,000 points: exactly 0 under a constant volume upstream, 4.9e-17 under the
first-moment one."""
import numpy as np
import pytest
import torch

from tests import cell_box_grad_ref as R
from tests.host_harness import clip_box_grad_host as BG
from tests.host_harness import clip_box_host as B
from tests.host_harness import clip_host as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_GPU = {}
_FD = {}


def _tensors(points, offsets, adjacency):
    return (torch.from_numpy(points).to(DEV), torch.from_numpy(adjacency.astype(np.int64)).to(DEV).to(torch.uint32),
            torch.from_numpy(offsets.astype(np.int64)).to(DEV).to(torch.uint32))


def _forward(t, box) -> dict:
    import radfoam

    geo = radfoam.cell_geometry_in_box(*t, np.asarray(box).tolist())
    out = {k: getattr(geo, k).cpu().numpy() for k in geo._fields}
    out["geo"] = geo
    return out


def _up(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(DEV)


def _run_on(t):
    """run(c, out, gv, gc) of the shared checks, on the device; ``out`` is what _forward returned for the same case"""
    import radfoam

    def run(c, out, gv, gc):
        return radfoam.cell_geometry_in_box_grad(*t, c["box"].tolist(), out["geo"], _up(gv), _up(gc)).cpu().numpy()

    return run


def _case(c: dict) -> dict:
    t = _tensors(c["points"], c["offsets"], c["adjacency"])
    return dict(c=c, t=t, out=_forward(t, c["box"]), run=_run_on(t))


def _device(name) -> dict:
    """a case of clip_box_host on the device, once"""
    if name not in _GPU:
        _GPU[name] = _case(B.case(name))
    return _GPU[name]


def _fd(name) -> dict:
    """a difference-quotient case (the cloud on the 2^-16 grid) on the device, once"""
    if name not in _FD:
        _FD[name] = _case(R.recorded_case(name))
    return _FD[name]


# ---- the recorded difference quotients ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.FD_CASES))
def test_gradient_matches_the_recorded_difference_quotients(name):
    d, rec = _fd(name), R.recorded(name)
    assert d["out"]["nonempty"][rec["cells"]].all()
    grad = d["run"](d["c"], d["out"], rec["w"], rec["u"])
    R.check_against_reference(name, rec, grad)
    host = BG.host_run(d["c"], BG.host_forward(("fd", name), d["c"]), rec["w"], rec["u"])
    BG.check_rows_agree(name, grad, host)


def test_the_seams_of_the_lane_path():
    for k, gon in ((58, 14), (59, 15), (64, 15), (65, 16)):
        d = _fd(f"hub{k}")
        assert int(d["c"]["offsets"][1]) == k and (d["out"]["face_area"][:k] == 0.0).sum() == 6
        assert d["out"]["wall_area"][0, 1] > 0.0
    for name, pairs in (("ring16_cut", ((0, 1),)), ("ring17_cut", ((0, 1),)), ("redo_spread_cut", H.REDO_SPREAD_PAIRS)):
        d = _fd(name)
        assert d["out"]["nonempty"][np.array(pairs).reshape(-1)].all()
    assert sorted(set((np.array(H.REDO_SPREAD_PAIRS).reshape(-1) // 64).tolist())) == [0, 1, 3]


# ---- checks without a reference --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["uniform400", "tight", "wide", "disjoint", "offset", "grid_bisectors"])
def test_a_constant_volume_upstream_has_a_gradient_of_exactly_zero(name):
    d = _device(name)
    BG.check_partition_volume(d["c"], d["out"], d["run"])
    gv, gc = BG.unit_upstreams(d["out"])
    assert np.isfinite(d["run"](d["c"], d["out"], gv, gc)).all()


@pytest.mark.parametrize("name", ["uniform400", "tight", "wide", "offset", "disjoint"])
def test_the_first_moment_of_the_partition_is_fixed(name):
    d = _device(name)
    BG.check_partition_moment(d["c"], d["out"], d["run"])


@pytest.mark.parametrize("name", ["tight", "disjoint"])
def test_non_finite_upstreams_on_empty_cells_do_not_leak(name):
    d = _device(name)
    BG.check_empty_cells_are_ignored(d["c"], d["out"], d["run"], least=100)


@pytest.mark.parametrize("name", ["uniform400", "tight", "offset"])
def test_none_is_zero_and_the_two_upstreams_add(name):
    d = _device(name)
    BG.check_none_and_linearity(d["c"], d["out"], d["run"])


def test_cells_that_touch_no_wall_agree_with_cell_geometry_grad():
    import radfoam

    d = _device("wide")
    plain = radfoam.cell_geometry(*d["t"])

    def plain_grad(gv, gc):
        return radfoam.cell_geometry_grad(*d["t"], plain, _up(gv), _up(gc)).cpu().numpy()

    BG.check_agreement(d["c"], d["out"], d["out"]["wall_area"], plain.bounded.cpu().numpy(), d["run"], plain_grad)


@pytest.mark.parametrize("name", ["uniform400", "tight", "wide", "disjoint", "offset", "grid_bisectors"])
def test_the_device_agrees_with_the_host_build(name):
    """unit upstreams on the device's own forward, through both: per row to 1e-9"""
    d = _device(name)
    gv, gc = BG.unit_upstreams(d["out"], seed=4)
    BG.check_rows_agree(name, d["run"](d["c"], d["out"], gv, gc), BG.host_run(d["c"], d["out"], gv, gc))


def test_tiny_inputs():
    import radfoam

    for name, c in BG.tiny_cases().items():
        d = _case(c)
        BG.check_tiny(c, d["out"], d["run"])
    cube = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
    t = (torch.zeros((0, 3), device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV),
         torch.zeros(1, dtype=torch.int32, device=DEV))
    geo = radfoam.cell_geometry_in_box(*t, cube)
    none = radfoam.cell_geometry_in_box_grad(*t, cube, geo, None, None)
    assert none.shape == (0, 3) and none.dtype == torch.float64
    none = radfoam.cell_geometry_in_box_grad(*t, cube, geo, torch.zeros(0, device=DEV), torch.zeros((0, 3), device=DEV))
    assert none.shape == (0, 3)


# ---- refusals and input forms ------------------------------------------------------------------------------------------

def test_a_257_gon_raises_naming_a_cell_of_the_ring():
    """the ring face kept whole by the box; the forward refuses the cloud, so the geometry is made up"""
    import radfoam
    from radfoam_amd import foam

    pts = H._CLOUDS["ring257"]()
    off, adj = foam.delaunay_csr(pts)
    n = len(pts)
    t = _tensors(pts, off, adj)
    geo = radfoam.BoxedCellGeometry(torch.ones(n, dtype=torch.float64, device=DEV), t[0].double(),
                                    torch.ones(n, dtype=torch.bool, device=DEV), None, None)
    with pytest.raises(RuntimeError, match=r"cell_geometry_in_box_grad: cell (\d+) is not supported: a face outgrew 256 "
                                           r"vertices") as err:
        radfoam.cell_geometry_in_box_grad(*t, B.RING_BOX[:5] + (5.0,), geo, torch.ones(n, device=DEV), None)
    assert int(str(err.value).split("cell ")[1].split()[0]) < 2 + 257


def test_a_malformed_row_a_bad_box_and_a_wrong_geometry_raise():
    import radfoam

    d = _device("uniform400")
    c, t, geo = d["c"], d["t"], d["out"]["geo"]
    n = len(c["points"])
    gv = torch.ones(n, device=DEV)
    adj = c["adjacency"].astype(np.int64)
    adj[int(c["offsets"][40])] = 40          # the site itself in its own row
    with pytest.raises(RuntimeError, match=r"cell_geometry_in_box_grad: cell 40 is not supported: its adjacency row is "
                                           r"malformed"):
        radfoam.cell_geometry_in_box_grad(t[0], torch.from_numpy(adj).to(DEV), t[2], c["box"], geo, gv, None)
    for bad in ((0, 0, 0, 1, 0, 1), (0, 0, 0, 1, float("nan"), 1), (0, 0, 0, 1, 1), torch.zeros(2, 3, device=DEV)):
        with pytest.raises(ValueError, match="box must"):
            radfoam.cell_geometry_in_box_grad(*t, bad, geo, gv, None)
        with pytest.raises(ValueError, match="box must"):
            radfoam.differentiable_cell_geometry_in_box(*t, bad)
    other = _device("wide")["out"]["geo"]._replace(volume=geo.volume[:-1])
    for wrong in (other, geo._replace(centroid=geo.centroid.float()), geo._replace(nonempty=geo.nonempty.to(torch.uint8)),
                  geo._replace(volume=geo.volume.cpu()), None):
        with pytest.raises(RuntimeError, match="geometry must be the BoxedCellGeometry"):
            radfoam.cell_geometry_in_box_grad(*t, c["box"], wrong, gv, None)
    with pytest.raises(RuntimeError, match="grad_volume must be a floating-point CUDA tensor of shape"):
        radfoam.cell_geometry_in_box_grad(*t, c["box"], geo, gv[:-1], None)
    with pytest.raises(RuntimeError, match="grad_centroid must be a floating-point CUDA tensor of shape"):
        radfoam.cell_geometry_in_box_grad(*t, c["box"], geo, None, torch.ones((n, 3), dtype=torch.int32, device=DEV))


def test_index_dtypes_box_forms_upstream_dtypes_and_repeat_runs_give_the_same_bits():
    import radfoam

    d, rec = _fd("ring17_cut"), R.recorded("ring17_cut")
    t, box, geo = d["t"], d["c"]["box"], d["out"]["geo"]
    w, u = _up(rec["w"].astype(np.float32)), _up(rec["u"].astype(np.float32))       # values fp32 holds exactly
    want = radfoam.cell_geometry_in_box_grad(*t, box, geo, w, u)
    same = lambda got: torch.equal(got, want)
    assert same(radfoam.cell_geometry_in_box_grad(*t, box, geo, w, u))                                   # two calls
    assert same(radfoam.cell_geometry_in_box_grad(*t, torch.from_numpy(box).reshape(2, 3).to(DEV), geo, w, u))
    assert same(radfoam.cell_geometry_in_box_grad(*t, box, geo, w.float(), u.float()))                  # f32 upstreams
    for dtype in (torch.int32, torch.int64):                                                           # next to uint32
        assert same(radfoam.cell_geometry_in_box_grad(t[0], t[1].to(dtype), t[2].to(dtype), box, geo, w, u))


# ---- device only -------------------------------------------------------------------------------------------------------

def test_the_wrapper_is_the_forward_bit_for_bit_and_autograd_is_the_operator():
    import radfoam

    d, rec = _fd("hub65"), R.recorded("hub65")
    t, box, out = d["t"], d["c"]["box"], d["out"]
    w, u = _up(rec["w"]), _up(rec["u"])
    points = t[0].clone().requires_grad_(True)
    geo = radfoam.differentiable_cell_geometry_in_box(points, t[1], t[2], box)
    assert isinstance(geo, radfoam.BoxedCellGeometry)
    for k in geo._fields:
        assert np.array_equal(getattr(geo, k).detach().cpu().numpy(), out[k], equal_nan=True)
    assert geo.volume.requires_grad and geo.centroid.requires_grad
    assert not geo.nonempty.requires_grad and not geo.face_area.requires_grad and not geo.wall_area.requires_grad
    ne = geo.nonempty
    ((w[ne] * geo.volume[ne]).sum() + (u[ne] * geo.centroid[ne]).sum()).backward()
    want = radfoam.cell_geometry_in_box_grad(*t, box, out["geo"], w, u)
    assert points.grad.dtype == torch.float32 and torch.equal(points.grad, want.to(torch.float32))
    # an output the loss leaves out arrives as None: the volume alone equals grad_centroid=None
    points.grad = None
    geo = radfoam.differentiable_cell_geometry_in_box(points, t[1], t[2], box)
    (w * geo.volume).sum().backward()
    assert torch.equal(points.grad, radfoam.cell_geometry_in_box_grad(*t, box, out["geo"], w, None).to(torch.float32))


def test_the_gpu_triangulation_feeds_straight_in():
    """20,000 uniform points, the GPU's own CSR, in [-1,1]^3: finite, exactly zero under check 1, and check 2"""
    import radfoam
    from radfoam_amd.triangulation import Triangulation

    gen = torch.Generator(device="cpu").manual_seed(0)
    start = (torch.rand((20000, 3), generator=gen) * 2.0 - 1.0).to(DEV)
    tri = Triangulation(start)
    points = start[tri.permutation().to(torch.int64)].contiguous()
    t = (points, tri.point_adjacency(), tri.point_adjacency_offsets())
    c = dict(points=points.cpu().numpy(), box=np.array([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]), name="triangulation 20000")
    out, run = _forward(t, c["box"]), _run_on(t)
    assert out["nonempty"].all()
    gv, gc = BG.unit_upstreams(out)
    assert np.isfinite(run(c, out, gv, gc)).all()
    BG.check_partition_volume(c, out, run)
    BG.check_partition_moment(c, out, run)


def test_the_example_descends_the_lloyd_energy_and_keeps_the_partition():
    from examples import foam_cvt_box as E

    rows = E.run(num_points=4000, steps=4, device=DEV, quiet=True)
    assert len(rows) == 4
    for ratio, energy, finite in rows:
        assert finite and abs(ratio - 1.0) <= 1e-9 and np.isfinite(energy)
    assert rows[-1][1] < rows[0][1]
