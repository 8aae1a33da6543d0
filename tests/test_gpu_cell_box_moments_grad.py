"""Point gradients of the boxed second moments on the GPU (radfoam.cell_moments_in_box_grad and
radfoam.differentiable_cell_moments_in_box, the kernels of rf_cell_box_moments_grad.hip) through the checks of
tests/test_cell_box_moments_grad.py (tests/host_harness/clip_box_moments_grad_host): the recorded difference quotients of
the exact rational boxed moments (tests/golden/cell_box_moments_grad/fd.npz; the rational code is not run here), the
closed forms and identities of a partition of a fixed box, agreement with cell_moments_grad away from the walls and with
the host build row by row, the seams between the lane-per-face kernel and the serial one, refusals, input forms, and the
autograd wrapper with its one fused launch.

Rows of up to 64 faces (lists of up to 70 planes) whose row polygons stay within 16 vertices are on the wave-per-cell
kernel: hub58, hub59 and hub64's site 0 and ring16_cut's axis sites.  hub65's site 0 (65 faces), ring17_cut's axis sites
and redo_spread_cut's eight (blocks 0, 1 and 3 of the redo kernel) go through the serial one.

Measured on the MI355X, worst |<grad, delta> - R| / spread (no probe needed the floor): uniform400 4.7e-6, tight 1.7e-5,
hub58 1.1e-3, hub59 1.4e-2, hub64 2.7e-3, hub65 3.5e-2, ring16_cut 2.8e-3, ring17_cut 1.7e-3, redo_spread_cut 3.2e-3; the
CVT closed form at most 1.8e-13 (tight) of the row scale; the partition through autograd at most 1.8e-15 (disjoint) of
sum |rows of the moment half|; the central path through autograd 1.2e-11 (tight); fusion 4.2e-14 (tight); against
cell_moments_grad on wide 2.3e-12; device against host build per row at most 2.5e-15; the GPU triangulation of 4,000
points: closed form 2.7e-16, partition 6.6e-17."""
import numpy as np
import pytest
import torch

from tests import cell_box_moments_grad_ref as R
from tests.host_harness import clip_box_host as B
from tests.host_harness import clip_box_moments_grad_host as MG
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
    """run(c, out, gq, gm, gv, gc) of the shared checks, on the device; ``out`` is what _forward returned for the case"""
    import radfoam

    def run(c, out, gq, gm, gv, gc):
        return radfoam.cell_moments_in_box_grad(*t, np.asarray(c["box"]).tolist(), out["geo"], _up(gq), _up(gm), _up(gv),
                                                _up(gc)).cpu().numpy()

    return run


def _geometry_run_on(t):
    import radfoam

    def run(c, out, gv, gc):
        return radfoam.cell_geometry_in_box_grad(*t, np.asarray(c["box"]).tolist(), out["geo"], _up(gv),
                                                 _up(gc)).cpu().numpy()

    return run


def _case(c: dict) -> dict:
    t = _tensors(c["points"], c["offsets"], c["adjacency"])
    return dict(c=c, t=t, out=_forward(t, c["box"]), run=_run_on(t), geometry_run=_geometry_run_on(t))


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


# ---- 1. the recorded difference quotients, and (g) on the same cases ---------------------------------------------------

@pytest.mark.parametrize("name", list(R.FD_CASES))
def test_gradient_matches_the_recorded_difference_quotients(name):
    d, rec = _fd(name), R.recorded(name)
    assert d["out"]["nonempty"][rec["cells"]].all()
    ups = (rec["A"], rec["B"], rec["w"], rec["u"])
    grad = d["run"](d["c"], d["out"], *ups)
    R.check_against_reference(name, rec, grad)
    host = MG.host_run(d["c"], MG.host_forward(("fd", name), d["c"]), *ups)
    MG.check_rows_agree(name, grad, host)


def test_the_seams_of_the_lane_path():
    """(h) on the device's forward: the rows that straddle the lane path's limits are what the cases say they are"""
    for k in (58, 59, 64, 65):
        d = _fd(f"hub{k}")
        assert int(d["c"]["offsets"][1]) == k and (d["out"]["face_area"][:k] == 0.0).sum() == 6
        assert d["out"]["wall_area"][0, 1] > 0.0
    for name, pairs in (("ring16_cut", ((0, 1),)), ("ring17_cut", ((0, 1),)), ("redo_spread_cut", H.REDO_SPREAD_PAIRS)):
        d = _fd(name)
        assert d["out"]["nonempty"][np.array(pairs).reshape(-1)].all()
    assert sorted(set((np.array(H.REDO_SPREAD_PAIRS).reshape(-1) // 64).tolist())) == [0, 1, 3]


# ---- 2. closed forms and identities ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", MG.PLAIN_CASES)
def test_the_trace_upstream_gives_the_cvt_gradient_on_every_nonempty_cell(name):
    """(a)"""
    d = _device(name)
    MG.check_cvt(d["c"], d["out"], d["run"])


def test_the_cvt_gradient_is_finite_where_walls_coincide_with_bisectors():
    d = _device("grid_bisectors")
    MG.check_cvt(d["c"], d["out"], d["run"], finite_only=True)


def _through_autograd(d, loss_of):
    """``loss_of(moments, p) -> scalar`` with ``moments`` what the wrapper returned for the case's float32 points and ``p``
    the same points as a float64 leaf, for the terms torch forms itself.  Returns (loss, total f64[N,3]): torch autograd
    gives the loss's own upstreams of the wrapper's four differentiable outputs and its direct term d loss / d p; the
    fused operator is launched once with those upstreams, and ``total`` is its rows plus the direct term, in double.
    The wrapper hands its gradient back in the dtype of ``points``, float32, so the double comparison is made on
    ``total``, and the wrapper's own ``.backward()`` must give the operator's rows rounded to float32, bit for bit."""
    import radfoam

    box = np.asarray(d["c"]["box"]).tolist()
    points = d["t"][0].clone().requires_grad_(True)
    p = d["t"][0].double().requires_grad_(True)
    mom = radfoam.differentiable_cell_moments_in_box(points, d["t"][1], d["t"][2], box)
    loss = loss_of(mom, p)
    outs = [mom.site_moment, mom.central_moment, mom.geometry.volume, mom.geometry.centroid]
    *ups, direct = torch.autograd.grad(loss, outs + [p], allow_unused=True, retain_graph=True)
    assert any(u is not None for u in ups[:2])
    fused = radfoam.cell_moments_in_box_grad(*d["t"], box, d["out"]["geo"], *ups)
    loss.backward()
    assert points.grad.dtype == torch.float32 and torch.equal(points.grad, fused.to(torch.float32))
    if direct is not None:
        assert torch.equal(p.grad, direct)
    total = fused if direct is None else fused + direct
    assert torch.isfinite(total).all()
    return loss.detach(), total


def _partition_check(d, name) -> float:
    """(b) through the wrapper and torch autograd: sum_a <G, Q_a> + 2 V_a q_a^T G (c_a - p_a) + V_a q_a^T G q_a is the
    constant <G, V_box diag(e^2 / 12)>, q_a = p_a - centre formed in torch from the points; its gradient, the fused launch
    plus torch's own direct terms, is zero to 1e-9 of sum |rows of the moment half alone|"""
    import radfoam

    box = np.asarray(d["c"]["box"], dtype=np.float64)
    e = box[3:] - box[:3]
    centre = torch.from_numpy(0.5 * (box[:3] + box[3:])).to(DEV)
    n = len(d["c"]["points"])
    worst = 0.0
    for g6 in MG.PARTITION_G:
        G, g6t = torch.from_numpy(MG.symmetric(g6)).to(DEV), torch.from_numpy(g6).to(DEV)

        def loss_of(mom, p):
            ne = mom.geometry.nonempty
            q, m, vol = p[ne] - centre, mom.geometry.centroid[ne] - p[ne], mom.geometry.volume[ne]
            return ((mom.site_moment[ne] * g6t).sum() + (2.0 * vol * ((q @ G) * m).sum(1)).sum()
                    + (vol * ((q @ G) * q).sum(1)).sum())

        loss, total = _through_autograd(d, loss_of)
        want = float((np.diag(MG.symmetric(g6)) * e.prod() * e * e / 12.0).sum())
        assert abs(loss.item() - want) <= 1e-9 * e.prod() * (e * e).sum()
        half = radfoam.cell_moments_in_box_grad(*d["t"], box.tolist(), d["out"]["geo"], g6t.expand(n, 6).contiguous())
        unit = half.norm(dim=1).sum().item()
        assert unit > 0.0
        ratio = total.norm(dim=1).max().item() / unit
        print(f"{name}: G = {g6.tolist()}: through autograd max |grad| = {total.norm(dim=1).max().item():.3g}, sum |rows of "
              f"the moment half| = {unit:.3g}, ratio {ratio:.3g} (bar {MG.ROW_BAR:.3g})")
        assert ratio <= MG.ROW_BAR
        worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("name", MG.PLAIN_CASES)
def test_the_second_moment_of_the_partition_is_fixed(name):
    """(b): through the wrapper and torch autograd, and the shared check with the direct terms formed by hand"""
    d = _device(name)
    _partition_check(d, name)
    MG.check_partition(d["c"], d["out"], d["run"])


@pytest.mark.parametrize("name", MG.PLAIN_CASES)
def test_the_central_path_equals_the_site_path_minus_the_shift(name):
    """(c): through the wrapper and torch autograd, the gradient of sum <H_a, central_a> against that of
    sum <H_a, site_a> - V_a m_a^T H_a m_a with m_a = c_a - p_a formed in torch from the wrapper's volume and centroid,
    random H = r / s^4: per row to 1e-9 of max(1, |row|); then the shared check with the direct terms formed by hand"""
    d = _device(name)
    ne_np = d["out"]["nonempty"].astype(bool)
    h6 = np.where(ne_np[:, None], MG.unit_upstreams(d["out"], seed=7)[1], 0.0)
    h6t, H = _up(h6), torch.from_numpy(MG.symmetric(h6)).to(DEV)

    def central(mom, p):
        ne = mom.geometry.nonempty
        return (mom.central_moment[ne] * h6t[ne]).sum()

    def site(mom, p):
        ne = mom.geometry.nonempty
        m = mom.geometry.centroid[ne] - p[ne]
        return (mom.site_moment[ne] * h6t[ne]).sum() - (mom.geometry.volume[ne] * torch.einsum("ni,nij,nj->n", m, H[ne], m)).sum()

    (l1, g1), (l2, g2) = _through_autograd(d, central), _through_autograd(d, site)
    assert g1.abs().max() > 0
    ratio = float(((g1 - g2).norm(dim=1) / g1.norm(dim=1).clamp(min=1.0)).max())
    print(f"{name}: central path through autograd: losses {l1.item():.12g} and {l2.item():.12g}, worst |difference| / row "
          f"scale = {ratio:.3g} (bar {MG.ROW_BAR:.3g})")
    assert ratio <= MG.ROW_BAR
    MG.check_central_path(d["c"], d["out"], d["run"])


@pytest.mark.parametrize("name", MG.PLAIN_CASES)
def test_the_fused_call_is_the_sum_of_its_halves_and_none_is_zero(name):
    """(d)"""
    d = _device(name)
    MG.check_fusion(d["c"], d["out"], d["run"], d["geometry_run"])


def test_cells_that_touch_no_wall_agree_with_cell_moments_grad():
    """(e)"""
    import radfoam

    d = _device("wide")
    plain = radfoam.cell_geometry(*d["t"])

    def plain_grad(gq, gm):
        return radfoam.cell_moments_grad(*d["t"], plain, _up(gq), _up(gm)).cpu().numpy()

    MG.check_agreement(d["c"], d["out"], plain.bounded.cpu().numpy(), d["run"], plain_grad)


@pytest.mark.parametrize("name", ["tight", "disjoint"])
def test_non_finite_upstreams_on_empty_cells_do_not_leak(name):
    """(f)"""
    d = _device(name)
    MG.check_empty_cells_are_ignored(d["c"], d["out"], d["run"], least=100)


@pytest.mark.parametrize("name", MG.PLAIN_CASES + ("grid_bisectors",))
def test_the_device_agrees_with_the_host_build(name):
    """(g): unit upstreams on the device's own forward, through both: per row to 1e-9"""
    d = _device(name)
    ups = MG.unit_upstreams(d["out"], seed=4)
    MG.check_rows_agree(name, d["run"](d["c"], d["out"], *ups), MG.host_run(d["c"], d["out"], *ups))


# ---- (i) tiny and malformed inputs ---------------------------------------------------------------------------------------

def test_tiny_inputs():
    import radfoam

    for name, c in MG.tiny_cases().items():
        d = _case(c)
        MG.check_tiny(c, d["out"], d["run"])
    cube = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
    t = (torch.zeros((0, 3), device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV),
         torch.zeros(1, dtype=torch.int32, device=DEV))
    geo = radfoam.cell_geometry_in_box(*t, cube)
    none = radfoam.cell_moments_in_box_grad(*t, cube, geo)
    assert none.shape == (0, 3) and none.dtype == torch.float64
    none = radfoam.cell_moments_in_box_grad(*t, cube, geo, torch.zeros((0, 6), device=DEV), None,
                                            torch.zeros(0, device=DEV), torch.zeros((0, 3), device=DEV))
    assert none.shape == (0, 3)


def test_an_emptied_row_leaves_every_other_rows_bits():
    import radfoam

    d = _device("uniform400")
    c, out, t = d["c"], d["out"], d["t"]
    a = 40
    off = c["offsets"].astype(np.int64)
    lo, hi = int(off[a]), int(off[a + 1])
    adj2 = np.concatenate([c["adjacency"][:lo], c["adjacency"][hi:]])
    off2 = off.copy()
    off2[a + 1:] -= hi - lo
    ups = [_up(u) for u in MG.unit_upstreams(out, seed=6)]
    full = radfoam.cell_moments_in_box_grad(*t, c["box"].tolist(), out["geo"], *ups)
    cut = radfoam.cell_moments_in_box_grad(t[0], torch.from_numpy(adj2.astype(np.int64)).to(DEV),
                                           torch.from_numpy(off2).to(DEV), c["box"].tolist(), out["geo"], *ups)
    rest = torch.arange(len(c["points"]), device=DEV) != a
    assert torch.equal(cut[rest], full[rest]) and torch.isfinite(cut).all()
    G = MG.symmetric(ups[0][a].cpu().numpy())
    want = -2.0 * out["volume"][a] * G @ (out["centroid"][a] - c["points"][a].astype(np.float64))
    assert np.abs(cut[a].cpu().numpy() - want).max() <= 1e-12 * np.abs(want).max()


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
    with pytest.raises(RuntimeError, match=r"cell_moments_in_box_grad: cell (\d+) is not supported: a face outgrew 256 "
                                           r"vertices") as err:
        radfoam.cell_moments_in_box_grad(*t, B.RING_BOX[:5] + (5.0,), geo, torch.ones((n, 6), device=DEV))
    assert int(str(err.value).split("cell ")[1].split()[0]) < 2 + 257


def test_a_malformed_row_a_bad_box_and_a_wrong_geometry_raise():
    import radfoam

    d = _device("uniform400")
    c, t, geo = d["c"], d["t"], d["out"]["geo"]
    n = len(c["points"])
    gq = torch.ones((n, 6), device=DEV)
    adj = c["adjacency"].astype(np.int64)
    adj[int(c["offsets"][40])] = 40          # the site itself in its own row
    with pytest.raises(RuntimeError, match=r"cell_moments_in_box_grad: cell 40 is not supported: its adjacency row is "
                                           r"malformed"):
        radfoam.cell_moments_in_box_grad(t[0], torch.from_numpy(adj).to(DEV), t[2], c["box"], geo, gq)
    for bad in ((0, 0, 0, 1, 0, 1), (0, 0, 0, 1, float("nan"), 1), (0, 0, 0, 1, 1), torch.zeros(2, 3, device=DEV)):
        with pytest.raises(ValueError, match="box must"):
            radfoam.cell_moments_in_box_grad(*t, bad, geo, gq)
        with pytest.raises(ValueError, match="box must"):
            radfoam.differentiable_cell_moments_in_box(*t, bad)
    other = _device("wide")["out"]["geo"]._replace(volume=geo.volume[:-1])
    for wrong in (other, geo._replace(centroid=geo.centroid.float()), geo._replace(nonempty=geo.nonempty.to(torch.uint8)),
                  geo._replace(volume=geo.volume.cpu()), None, "geometry"):
        with pytest.raises(RuntimeError, match="geometry must be the BoxedCellGeometry"):
            radfoam.cell_moments_in_box_grad(*t, c["box"], wrong, gq)
    with pytest.raises(RuntimeError, match="grad_site_moment must be a floating-point CUDA tensor of shape"):
        radfoam.cell_moments_in_box_grad(*t, c["box"], geo, gq[:-1])
    with pytest.raises(RuntimeError, match="grad_central_moment must be a floating-point CUDA tensor of shape"):
        radfoam.cell_moments_in_box_grad(*t, c["box"], geo, None, torch.ones((n, 6), dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="grad_centroid must be a floating-point CUDA tensor of shape"):
        radfoam.cell_moments_in_box_grad(*t, c["box"], geo, gq, None, None, torch.ones((n, 2), device=DEV))


def test_index_dtypes_box_forms_upstream_dtypes_and_repeat_runs_give_the_same_bits():
    import radfoam

    d, rec = _fd("ring17_cut"), R.recorded("ring17_cut")
    t, box, geo = d["t"], d["c"]["box"], d["out"]["geo"]
    ups = [_up(rec[k].astype(np.float32)) for k in ("A", "B", "w", "u")]       # values fp32 holds exactly
    want = radfoam.cell_moments_in_box_grad(*t, box, geo, *ups)
    same = lambda got: torch.equal(got, want)
    assert torch.isfinite(want).all() and want.abs().max() > 0
    assert same(radfoam.cell_moments_in_box_grad(*t, box, geo, *ups))                                   # two calls
    assert same(radfoam.cell_moments_in_box_grad(*t, torch.from_numpy(box).reshape(2, 3).to(DEV), geo, *ups))
    assert same(radfoam.cell_moments_in_box_grad(*t, box, geo, *[u.float() for u in ups]))              # f32 upstreams
    for dtype in (torch.int32, torch.int64):                                                           # next to uint32
        assert same(radfoam.cell_moments_in_box_grad(t[0], t[1].to(dtype), t[2].to(dtype), box, geo, *ups))


# ---- (j) the wrapper -------------------------------------------------------------------------------------------------------

def test_the_wrapper_is_the_forward_bit_for_bit_and_autograd_is_one_fused_launch(monkeypatch):
    import radfoam
    from radfoam_amd import geometry as GEO

    d = _fd("hub65")
    t, box, out = d["t"], d["c"]["box"].tolist(), d["out"]
    want = radfoam.cell_moments_in_box(*t, box)
    calls = []
    fused, plain = GEO._run_moments_in_box_grad, GEO._run_geometry_in_box_grad
    monkeypatch.setattr(GEO, "_run_moments_in_box_grad", lambda *a: calls.append("moments") or fused(*a))
    monkeypatch.setattr(GEO, "_run_geometry_in_box_grad", lambda *a: calls.append("geometry") or plain(*a))

    def wrapped():
        points = t[0].clone().requires_grad_(True)
        return points, radfoam.differentiable_cell_moments_in_box(points, t[1], t[2], box)

    points, mom = wrapped()
    assert isinstance(mom, radfoam.BoxedCellMoments) and isinstance(mom.geometry, radfoam.BoxedCellGeometry)
    assert torch.equal(mom.site_moment.detach(), want.site_moment)
    assert torch.equal(mom.central_moment.detach().nan_to_num(nan=-1.0), want.central_moment.nan_to_num(nan=-1.0))
    assert torch.equal(torch.isnan(mom.central_moment.detach()), torch.isnan(want.central_moment))
    for k in want.geometry._fields:
        assert np.array_equal(getattr(mom.geometry, k).detach().cpu().numpy(), out[k], equal_nan=True)
    assert all(x.requires_grad for x in (mom.site_moment, mom.central_moment, mom.geometry.volume, mom.geometry.centroid))
    assert not any(x.requires_grad for x in (mom.geometry.nonempty, mom.geometry.face_area, mom.geometry.wall_area))
    # sum tr site + sum tr central / V + sum w V: ONE launch of the fused operator, bitwise the operator called by hand
    # with the loss's own upstreams (what torch autograd hands the wrapper's outputs)
    ne = mom.geometry.nonempty
    w = _up(MG.unit_upstreams(out, seed=9)[2]).nan_to_num(nan=0.0)
    vol = mom.geometry.volume
    loss = mom.site_moment[ne, :3].sum() + (mom.central_moment[ne, :3].sum(1) / vol[ne]).sum() + (w[ne] * vol[ne]).sum()
    ups = torch.autograd.grad(loss, [mom.site_moment, mom.central_moment, vol], retain_graph=True)
    assert calls == []
    loss.backward()
    assert calls == ["moments"]
    by_hand = radfoam.cell_moments_in_box_grad(*t, box, out["geo"], *ups, None)
    assert points.grad.dtype == torch.float32 and torch.equal(points.grad, by_hand.to(torch.float32))
    assert torch.isfinite(by_hand).all() and by_hand.abs().max() > 0
    # only volume / centroid in the loss: cell_geometry_in_box_grad, bitwise differentiable_cell_geometry_in_box's gradient
    del calls[:]
    u = _up(MG.unit_upstreams(out, seed=9)[3]).nan_to_num(nan=0.0)
    points, mom = wrapped()
    ((w * mom.geometry.volume).sum() + (u[ne] * mom.geometry.centroid[ne]).sum()).backward()
    assert calls == ["geometry"]
    other = t[0].clone().requires_grad_(True)
    geo = radfoam.differentiable_cell_geometry_in_box(other, t[1], t[2], box)
    ((w * geo.volume).sum() + (u[ne] * geo.centroid[ne]).sum()).backward()
    assert torch.equal(points.grad, other.grad) and points.grad.abs().max() > 0
    # an output the loss leaves out triggers no launch
    del calls[:]
    points, mom = wrapped()
    (points * 2.0).sum().backward()
    assert calls == [] and torch.equal(points.grad, torch.full_like(points, 2.0))


def test_the_gpu_triangulation_feeds_straight_in():
    """end to end: 4,000 uniform points triangulated on the device, the box [-1,1]^3: all rows finite, (a) and (b)"""
    from radfoam_amd.triangulation import Triangulation

    gen = torch.Generator(device="cpu").manual_seed(0)
    start = (torch.rand((4000, 3), generator=gen) * 2.0 - 1.0).to(DEV)
    tri = Triangulation(start)
    points = start[tri.permutation().to(torch.int64)].contiguous()
    t = (points, tri.point_adjacency(), tri.point_adjacency_offsets())
    c = dict(points=points.cpu().numpy(), offsets=t[2].cpu().numpy().astype(np.int64),
             adjacency=t[1].cpu().numpy().astype(np.int64), box=np.array([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]),
             name="triangulation 4000")
    d = dict(c=c, t=t, out=_forward(t, c["box"]), run=_run_on(t))
    assert d["out"]["nonempty"].all()
    assert np.isfinite(d["run"](c, d["out"], *MG.unit_upstreams(d["out"]))).all()
    MG.check_cvt(c, d["out"], d["run"])
    MG.check_partition(c, d["out"], d["run"])
    _partition_check(d, c["name"])


def test_the_example_descends_the_cvt_energy_and_keeps_the_partition():
    from examples import foam_cvt_box as E

    rows = E.run(num_points=4000, steps=4, device=DEV, quiet=True, energy="cvt", aniso=0.1, equal_volume=0.5)
    assert len(rows) == 4
    for ratio, energy, finite in rows:
        assert finite and abs(ratio - 1.0) <= 1e-9 and np.isfinite(energy)
    rows = E.run(num_points=4000, steps=4, device=DEV, quiet=True, energy="cvt")
    assert all(finite for _, _, finite in rows) and rows[-1][1] < rows[0][1]
