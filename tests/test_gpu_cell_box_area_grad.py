"""Point gradients of the boxed face and wall areas on the GPU (radfoam.face_area_in_box_grad and
radfoam.differentiable_cell_geometry_in_box(..., face_area=True), the kernels of rf_cell_box_area_grad.hip) through the
checks of tests/test_cell_box_area_grad.py (tests/host_harness/clip_box_area_grad_host): the recorded difference
quotients of the exact rational boxed areas (tests/golden/cell_box_area_grad/fd.npz; the rational code is not run here),
the identities of the areas of a partition of a fixed box, agreement with face_area_grad away from the walls and with the
host build row by row, the seams between the lane-per-face kernel and the serial one, refusals, input forms and autograd.

Rows of up to 64 faces (lists of up to 70 planes) whose row polygons stay within 16 vertices are on the wave-per-cell
kernel: hub58, hub59 and hub64's site 0 and ring16_cut's axis sites.  hub65's site 0 (65 faces), ring17_cut's axis
sites and redo_spread_cut's eight (blocks 0, 1 and 3 of the redo kernel) go through the serial one.

Measured on the MI355X: see DESIGN.md, "Point gradients of the face and wall areas in a box"."""
import numpy as np
import pytest
import torch

from tests import cell_box_area_grad_ref as R
from tests.host_harness import clip_box_area_grad_host as A
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
    """run(c, out, g, gw) of the shared checks, on the device; ``out`` is what _forward returned for the same case"""
    import radfoam

    def run(c, out, g, gw):
        return radfoam.face_area_in_box_grad(*t, np.asarray(c["box"]).tolist(), out["geo"], _up(g), _up(gw)).cpu().numpy()

    return run


def _case(c: dict) -> dict:
    c = A.with_rows(c)
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
    assert (d["out"]["face_area"][rec["keep_slot"]] > 0).all() and (d["out"]["wall_area"][rec["keep_wall"]] > 0).all()
    grad = d["run"](d["c"], d["out"], rec["g"], rec["gw"])
    R.check_against_reference(name, rec, grad)
    host = A.host_run(d["c"], A.host_forward(("fd", name), d["c"]), rec["g"], rec["gw"])
    A.check_rows_agree(name, grad, host)


def test_the_seams_of_the_lane_path():
    for k in (58, 59, 64, 65):
        d = _fd(f"hub{k}")
        assert int(d["c"]["offsets"][1]) == k and (d["out"]["face_area"][:k] == 0.0).sum() == 6
        assert d["out"]["wall_area"][0, 1] > 0.0
    for name, pairs in (("ring16_cut", ((0, 1),)), ("ring17_cut", ((0, 1),)), ("redo_spread_cut", H.REDO_SPREAD_PAIRS)):
        d = _fd(name)
        assert d["out"]["nonempty"][np.array(pairs).reshape(-1)].all()
    assert sorted(set((np.array(H.REDO_SPREAD_PAIRS).reshape(-1) // 64).tolist())) == [0, 1, 3]


# ---- checks without a reference --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,exact", [("uniform400", True), ("wide", True), ("offset", True), ("tight", False),
                                        ("disjoint", False), ("grid_bisectors", False)])
def test_a_wall_upstream_constant_down_each_column_has_no_gradient(name, exact):
    d = _device(name)
    A.check_constant_wall_upstream(d["c"], d["out"], d["run"], exact)


@pytest.mark.parametrize("name", ["uniform400", "tight", "wide"])
def test_the_area_vectors_close_through_autograd(name):
    """check 2: sum_a u_a . (sum_b A_ab d^_ab + sum_w A_aw n_w), built with the wrapper and torch, is identically zero in
    the points; .backward() gives a gradient with sum |p_a| |grad_a| <= 1e-9 sum |p_a| |term_a|, term_a the operator's
    half alone (face_area_in_box_grad with the upstreams autograd hands it)"""
    import radfoam

    d = _device(name)
    c, t, out = d["c"], d["t"], d["out"]
    u = _up(A.closure_upstreams(c, out)[0])
    rows, adj = torch.from_numpy(c["rows"]).to(DEV), t[1].to(torch.int64)
    # the wrapper takes fp32 points and returns an fp32 gradient, so the operator's half is also read in double: the
    # upstreams autograd hands to the areas are caught by hooks and given to the operator, and the half through d^ flows
    # to a double copy of the points
    points, direct = t[0].clone().requires_grad_(True), t[0].double().requires_grad_(True)
    geo = radfoam.differentiable_cell_geometry_in_box(points, t[1], t[2], c["box"].tolist(), face_area=True)
    assert geo.face_area.requires_grad and geo.wall_area.requires_grad
    caught = {}
    geo.face_area.register_hook(lambda x: caught.__setitem__("g", x.clone()))
    geo.wall_area.register_hook(lambda x: caught.__setitem__("gw", x.clone()))
    diff = direct[adj] - direct[rows]
    unit = diff / diff.norm(dim=1, keepdim=True)
    closed = torch.zeros_like(direct).index_add(0, rows, geo.face_area[:, None] * unit) + geo.wall_area @ _up(A.NORMALS)
    (u * closed).sum().backward()
    term = radfoam.face_area_in_box_grad(*t, c["box"].tolist(), out["geo"], caught["g"], caught["gw"])
    assert torch.equal(points.grad, term.to(torch.float32))          # what .backward() delivered is the operator
    grad, term = (term + direct.grad).cpu().numpy(), term.cpu().numpy()
    size = np.linalg.norm(c["points"].astype(np.float64), axis=1)
    top, scale = (size * np.linalg.norm(grad, axis=1)).sum(), (size * np.linalg.norm(term, axis=1)).sum()
    print(f"{name}: closure through autograd: {top:.3g} of {scale:.4g}: {top / scale:.3g} (bar {A.CLOSURE_BAR:.3g})")
    assert np.isfinite(grad).all() and scale > 0.0 and top <= A.CLOSURE_BAR * scale
    A.check_closure(c, out, d["run"])


def test_slots_away_from_the_walls_agree_with_face_area_grad():
    import radfoam

    d = _device("wide")
    plain = radfoam.cell_geometry(*d["t"])
    geo = dict(bounded=plain.bounded.cpu().numpy())

    def plain_grad(g):
        return radfoam.face_area_grad(*d["t"], plain, _up(g)).cpu().numpy()

    A.check_agreement(d["c"], d["out"], geo, d["run"], plain_grad)


@pytest.mark.parametrize("name", ["tight", "disjoint"])
def test_non_finite_upstreams_on_empty_cells_do_not_leak(name):
    d = _device(name)
    A.check_empty_cells_are_ignored(d["c"], d["out"], d["run"], least=100)


@pytest.mark.parametrize("name", ["uniform400", "tight", "offset"])
def test_none_is_zero_and_the_two_upstreams_add(name):
    d = _device(name)
    A.check_none_and_additivity(d["c"], d["out"], d["run"])


@pytest.mark.parametrize("name", ["uniform400", "tight", "wide", "disjoint", "offset", "grid_bisectors"])
def test_the_device_agrees_with_the_host_build(name):
    """unit upstreams on the device's own forward, through both: per row to 1e-9"""
    d = _device(name)
    g, gw = A.unit_upstreams(d["c"], d["out"], seed=4)
    A.check_rows_agree(name, d["run"](d["c"], d["out"], g, gw), A.host_run(d["c"], d["out"], g, gw))


def test_degenerate_clouds():
    import radfoam

    d = _device("grid_bisectors")
    assert np.isfinite(d["run"](d["c"], d["out"], *A.unit_upstreams(d["c"], d["out"]))).all()
    for name, c in A.tiny_cases().items():
        d = _case(c)
        A.check_tiny(d["c"], d["out"], d["run"])
    cube = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
    t = (torch.zeros((0, 3), device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV),
         torch.zeros(1, dtype=torch.int32, device=DEV))
    geo = radfoam.cell_geometry_in_box(*t, cube)
    none = radfoam.face_area_in_box_grad(*t, cube, geo)
    assert none.shape == (0, 3) and none.dtype == torch.float64
    none = radfoam.face_area_in_box_grad(*t, cube, geo, torch.zeros(0, device=DEV), torch.zeros((0, 6), device=DEV))
    assert none.shape == (0, 3)


# ---- refusals and input forms ------------------------------------------------------------------------------------------

def test_a_257_gon_raises_naming_a_cell_of_the_ring():
    """the ring face kept whole by the box; the forward refuses the cloud, so the geometry is made up"""
    import radfoam
    from radfoam_amd import foam

    pts = H._CLOUDS["ring257"]()
    off, adj = foam.delaunay_csr(pts)
    n, e = len(pts), len(adj)
    t = _tensors(pts, off, adj)
    geo = radfoam.BoxedCellGeometry(torch.ones(n, dtype=torch.float64, device=DEV), t[0].double(),
                                    torch.ones(n, dtype=torch.bool, device=DEV),
                                    torch.ones(e, dtype=torch.float64, device=DEV),
                                    torch.ones((n, 6), dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError, match=r"face_area_in_box_grad: cell (\d+) is not supported: a face outgrew 256 "
                                           r"vertices") as err:
        radfoam.face_area_in_box_grad(*t, B.RING_BOX[:5] + (5.0,), geo, torch.ones(e, device=DEV), None)
    assert int(str(err.value).split("cell ")[1].split()[0]) < 2 + 257


def test_a_malformed_row_a_bad_box_and_a_wrong_geometry_raise():
    import radfoam

    d = _device("uniform400")
    c, t, geo = d["c"], d["t"], d["out"]["geo"]
    n, e = len(c["points"]), len(c["adjacency"])
    g = torch.ones(e, device=DEV)
    adj = c["adjacency"].astype(np.int64)
    adj[int(c["offsets"][40])] = 40          # the site itself in its own row
    with pytest.raises(RuntimeError, match=r"face_area_in_box_grad: cell 40 is not supported: its adjacency row is "
                                           r"malformed"):
        radfoam.face_area_in_box_grad(t[0], torch.from_numpy(adj).to(DEV), t[2], c["box"], geo, g, None)
    for bad in ((0, 0, 0, 1, 0, 1), (0, 0, 0, 1, float("nan"), 1), (0, 0, 0, 1, 1), torch.zeros(2, 3, device=DEV)):
        with pytest.raises(ValueError, match="box must"):
            radfoam.face_area_in_box_grad(*t, bad, geo, g, None)
        with pytest.raises(ValueError, match="box must"):
            radfoam.differentiable_cell_geometry_in_box(*t, bad, face_area=True)
    for wrong in (geo._replace(face_area=geo.face_area[:-1]), geo._replace(wall_area=geo.wall_area[:, :5]),
                  geo._replace(wall_area=geo.wall_area.float()), geo._replace(volume=geo.volume[:-1]),
                  geo._replace(face_area=geo.face_area.cpu()), None):
        with pytest.raises(RuntimeError, match="geometry must be the BoxedCellGeometry"):
            radfoam.face_area_in_box_grad(*t, c["box"], wrong, g, None)
    with pytest.raises(RuntimeError, match="grad_face_area must be a floating-point CUDA tensor of shape"):
        radfoam.face_area_in_box_grad(*t, c["box"], geo, g[:-1], None)
    with pytest.raises(RuntimeError, match="grad_wall_area must be a floating-point CUDA tensor of shape"):
        radfoam.face_area_in_box_grad(*t, c["box"], geo, None, torch.ones((n, 6), dtype=torch.int32, device=DEV))


def test_index_dtypes_box_forms_upstream_dtypes_and_repeat_runs_give_the_same_bits():
    import radfoam

    d, rec = _fd("ring17_cut"), R.recorded("ring17_cut")
    t, box, geo = d["t"], d["c"]["box"], d["out"]["geo"]
    g, gw = _up(rec["g"].astype(np.float32)), _up(rec["gw"].astype(np.float32))       # values fp32 holds exactly
    want = radfoam.face_area_in_box_grad(*t, box, geo, g, gw)
    same = lambda got: torch.equal(got, want)
    assert want.abs().max() > 0
    assert same(radfoam.face_area_in_box_grad(*t, box, geo, g, gw))                                      # two calls
    assert same(radfoam.face_area_in_box_grad(*t, torch.from_numpy(box).reshape(2, 3).to(DEV), geo, g, gw))
    assert same(radfoam.face_area_in_box_grad(*t, box, geo, g.float(), gw.float()))                     # f32 upstreams
    for dtype in (torch.int32, torch.int64):                                                           # next to uint32
        assert same(radfoam.face_area_in_box_grad(t[0], t[1].to(dtype), t[2].to(dtype), box, geo, g, gw))


# ---- device only -------------------------------------------------------------------------------------------------------

def test_the_wrapper_is_the_forward_bit_for_bit_and_autograd_is_the_sum_of_the_two_operators(monkeypatch):
    import radfoam
    from radfoam_amd import geometry
    from tests import cell_box_grad_ref as BR

    d, rec, vol = _fd("hub65"), R.recorded("hub65"), BR.recorded("hub65")
    t, box, out = d["t"], d["c"]["box"], d["out"]
    g, gw, w, u = _up(rec["g"]), _up(rec["gw"]), _up(vol["w"]), _up(vol["u"])
    for flag in (False, True):
        points = t[0].clone().requires_grad_(True)
        geo = radfoam.differentiable_cell_geometry_in_box(points, t[1], t[2], box, face_area=flag)
        assert isinstance(geo, radfoam.BoxedCellGeometry)
        for k in geo._fields:
            assert np.array_equal(getattr(geo, k).detach().cpu().numpy(), out[k], equal_nan=True)
        assert geo.volume.requires_grad and geo.centroid.requires_grad and not geo.nonempty.requires_grad
        assert geo.face_area.requires_grad == flag and geo.wall_area.requires_grad == flag
    default = radfoam.differentiable_cell_geometry_in_box(t[0].clone().requires_grad_(True), t[1], t[2], box)
    assert not default.face_area.requires_grad and not default.wall_area.requires_grad          # as before the flag
    ne = geo.nonempty
    ((g * geo.face_area).sum() + (gw * geo.wall_area).sum() + (w[ne] * geo.volume[ne]).sum()
     + (u[ne] * geo.centroid[ne]).sum()).backward()
    first = radfoam.cell_geometry_in_box_grad(*t, box, out["geo"], w, u)
    second = radfoam.face_area_in_box_grad(*t, box, out["geo"], g, gw)
    assert second.abs().max() > 0
    assert points.grad.dtype == torch.float32 and torch.equal(points.grad, (first + second).to(torch.float32))
    # the areas alone: the new operator alone, and one upstream alone equals None for the other
    points.grad = None
    geo = radfoam.differentiable_cell_geometry_in_box(points, t[1], t[2], box, face_area=True)
    (gw * geo.wall_area).sum().backward()
    assert torch.equal(points.grad, radfoam.face_area_in_box_grad(*t, box, out["geo"], None, gw).to(torch.float32))
    # a loss that leaves the areas out does not launch the new kernels
    calls = []
    real = geometry._run_face_area_in_box_grad
    monkeypatch.setattr(geometry, "_run_face_area_in_box_grad", lambda *a: calls.append(1) or real(*a))
    points.grad = None
    geo = radfoam.differentiable_cell_geometry_in_box(points, t[1], t[2], box, face_area=True)
    (w * geo.volume).sum().backward()
    assert not calls
    assert torch.equal(points.grad, radfoam.cell_geometry_in_box_grad(*t, box, out["geo"], w, None).to(torch.float32))
    geo = radfoam.differentiable_cell_geometry_in_box(points, t[1], t[2], box, face_area=True)
    (g * geo.face_area).sum().backward()
    assert calls == [1]


def test_the_gpu_triangulation_feeds_straight_in():
    """20,000 uniform points, the GPU's own CSR, in [-1,1]^3: finite, exactly zero under check 1, and check 2"""
    from radfoam_amd.triangulation import Triangulation

    gen = torch.Generator(device="cpu").manual_seed(0)
    start = (torch.rand((20000, 3), generator=gen) * 2.0 - 1.0).to(DEV)
    tri = Triangulation(start)
    points = start[tri.permutation().to(torch.int64)].contiguous()
    t = (points, tri.point_adjacency(), tri.point_adjacency_offsets())
    c = A.with_rows(dict(points=points.cpu().numpy(), adjacency=t[1].cpu().numpy(), offsets=t[2].cpu().numpy(),
                         box=np.array([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]), name="triangulation 20000"))
    out, run = _forward(t, c["box"]), _run_on(t)
    assert out["nonempty"].all()
    grad = run(c, out, *A.unit_upstreams(c, out))
    assert np.isfinite(grad).all() and (np.abs(grad).max(1) > 0).all()          # every site, the hull included
    A.check_constant_wall_upstream(c, out, run, exact=True)
    A.check_closure(c, out, run)


def test_the_example_reaches_every_face_with_the_box():
    from examples import foam_tv_box as E

    rows = E.run(num_points=4000, steps=3, device=DEV, quiet=True)
    assert len(rows) == 3
    for loss, boxed, unboxed, finite, rescued in rows:
        assert finite and np.isfinite(loss) and unboxed <= boxed and boxed >= 0.99 * 4000
        assert rescued > 0          # the hull's unbounded faces carry weight only in the box
    assert rows[-1][0] < rows[0][0]
