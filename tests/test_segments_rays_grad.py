"""CPU: radfoam.segment_rays_grad (the vectorised torch restatement of DESIGN 4.10) on segments of the CPU oracle, as
tests/test_segments_grad.py has them: against autograd of the definition, central differences, the invariants of the
direction gradient, the holder rule, a case small enough to do by hand, the entries that must add nothing, and the
autograd function Pipeline.trace_differentiable_segments uses."""
import numpy as np
import torch

import radfoam
from radfoam import composite_segments, segment_points_grad, segment_rays_grad
from tests import helpers as H
from tests import segments_grad_ref as G
from tests import segments_ref as S

INF = float("inf")


def _case(foam_factory, **settings):
    """(fm, rays [R, 6], oracle dict, exit_cells uint32 [R]) of the image case under `settings`."""
    fm, rays, _, full = S.image_case(foam_factory)
    short = S.image_case(foam_factory, **settings)[3] if settings else full
    return fm, rays.reshape(-1, 6), short, G.exit_cells_from_longer_walk(short, full)


def _subset(ref, exit_cells, rays, which):
    """The rays `which` of an oracle dict as a torch seg dict, with their exit cells and ray rows."""
    entries = np.concatenate([np.arange(ref["offsets"][r], ref["offsets"][r + 1]) for r in which])
    seg = {"offsets": torch.from_numpy(np.concatenate([[0], np.cumsum(ref["counts"][which])]).astype(np.int64)),
           "cells": torch.from_numpy(ref["cells"][entries]), "t_exit": torch.from_numpy(ref["t_exit"][entries]),
           "t_enter": torch.from_numpy(ref["t_enter"][entries])}
    return seg, exit_cells[which], rays[which]


_EIGHTH = {}


def _eighth(foam_factory):
    """Every 8th ray of the weight_threshold = 0.5 frame with what the composited loss needs, computed once."""
    if not _EIGHTH:
        fm, rays, ref, exits = _case(foam_factory, weight_threshold=0.5)
        seg, exits, rays = _subset(ref, exits, rays, np.arange(0, len(ref["counts"]), 8))
        rng = np.random.default_rng(7)
        density = torch.from_numpy(fm["attributes"][:, -1].astype(np.float64)) + 0.2    # no empty cells
        _EIGHTH["case"] = {
            "seg": seg, "exits": exits, "rays": torch.from_numpy(rays).double(),
            "points": torch.from_numpy(fm["points"]).double(), "density": density,
            "rgb": torch.from_numpy(rng.uniform(0.0, 1.0, size=(density.numel(), 3))),
            "weights": torch.from_numpy(rng.normal(size=(len(rays), 4))),
            "held_by": G.holders_by_loop(seg["offsets"].numpy(), seg["t_exit"].numpy()),
            "after": G.next_cells(seg, exits)}
    return _EIGHTH["case"]


def _loss(c, t_enter, t_exit):
    return (composite_segments({**c["seg"], "t_enter": t_enter, "t_exit": t_exit}, c["density"], c["rgb"])
            * c["weights"]).sum()


def _restated_from_graph(c, rays):
    """(rays.grad by autograd through exact_times, the restatement fed t_enter.grad / t_exit.grad of the same graph)."""
    rays = rays.clone().requires_grad_(True)
    # clones, so that t_exit.grad is the gradient of t_exit as composited alone: in exact_times' graph t_enter is made
    # of t_exit, and the restatement does that step itself (the holder rule)
    t_enter, t_exit = (t.clone() for t in G.exact_times(c["points"], rays, c["seg"], c["after"], c["held_by"]))
    t_enter.retain_grad()
    t_exit.retain_grad()
    _loss(c, t_enter, t_exit).backward()
    got = segment_rays_grad(c["seg"], torch.from_numpy(c["exits"]), c["points"], rays.detach(), t_enter.grad,
                            t_exit.grad)
    return rays.grad, got


def test_against_autograd_of_the_definition(foam_factory):
    """Every 8th ray of the weight_threshold = 0.5 frame (384 rays).  segments_grad_ref.exact_times is the definition in
    torch: fed float64 rays that require grad and composited (density + 0.2, random colour, random weights),
    rays.grad by autograd is the reference; the restatement gets t_enter.grad / t_exit.grad of the same graph.  Both
    sides are float64 evaluations of the same function: helpers.grad_close at rtol = 1e-6.  Measured: relative L2
    1.9e-16, worst element at 4.9e-10 of that bound."""
    c = _eighth(foam_factory)
    want, got = _restated_from_graph(c, c["rays"])
    assert got.dtype == torch.float64 and got.shape == want.shape == (384, 6)
    assert bool(torch.isfinite(want).all()) and bool((want != 0).any(dim=1).all())
    ok, rel, worst = H.grad_close(got.numpy(), want.numpy(), rtol=1e-6)
    print("relative L2 to autograd of the definition %.3g, worst element at %.3g of the bound" % (rel, worst))
    assert ok, worst


def test_central_differences(foam_factory):
    """All six components of four rays of that frame, one with a finite last exit and one with a non-holder entry among
    them: 24 coordinates.  The protocol of tests/test_segments_grad.py: the function differenced is the float64 loss
    over the exact bisector times of the fixed cell sequence; the step is the one of 2^-16 .. 2^-23 at which halving
    changes the estimates least, and the bar is twice that change.  Measured: step 2^-21 = 4.8e-7, change on halving
    5.6e-7 (2.3e-2 at 2^-20, where a step still crosses the kink of a zero-length interval; 4.8e-6 at 2^-23), difference
    to the restatement 3.4e-7, on gradients of up to 12.6."""
    c = _eighth(foam_factory)
    seg, off = c["seg"], c["seg"]["offsets"].numpy()
    last = seg["t_exit"][seg["offsets"][1:] - 1].numpy()
    non_holder = (seg["t_exit"] <= seg["t_enter"]).numpy()
    with_non_holder = [r for r in range(len(off) - 1) if non_holder[off[r]:off[r + 1]].any()]
    finite_last = [r for r in range(len(off) - 1) if np.isfinite(last[r])]
    assert with_non_holder and finite_last
    chosen = [finite_last[0], with_non_holder[0]]
    chosen += [r for r in (5, 200, 383, 100) if r not in chosen][:2]
    coords = [(r, a) for r in chosen for a in range(6)]
    assert len(coords) == 24

    _, got = _restated_from_graph(c, c["rays"])
    want = np.array([float(got[r, a]) for r, a in coords])
    assert (want != 0).sum() >= 22

    def central(h):
        out = []
        for r, a in coords:
            moved = []
            for sign in (1.0, -1.0):
                rays = c["rays"].clone()
                rays[r, a] += sign * h
                moved.append(float(_loss(c, *G.exact_times(c["points"], rays, seg, c["after"], c["held_by"]))))
            out.append((moved[0] - moved[1]) / (2.0 * h))
        return np.array(out)

    steps = [2.0 ** -k for k in range(16, 25)]
    estimates = [central(h) for h in steps]
    change = [float(np.abs(a - b).max()) for a, b in zip(estimates[:-1], estimates[1:])]
    best = int(np.argmin(change))
    print("change on halving, step by step:", ["%.2g" % x for x in change])
    error = float(np.abs(estimates[best] - want).max())
    print("step %.3g: change on halving %.3g, difference to the restatement %.3g, largest gradient %.3g"
          % (steps[best], change[best], error, np.abs(want).max()))
    assert change[best] < 1e-5 * np.abs(want).max()
    assert error <= 2.0 * change[best]


_FLAT = {}


def _flat(foam_factory):
    """300 incoherent un-normalised rays (helpers.random_rays) through foam_factory(6000, 0, 11), the oracle's
    segments."""
    if not _FLAT:
        fm = foam_factory(6000, 0, 11)
        rays, starts = H.random_rays(fm, 300, seed=3)
        ref = S.oracle_segments(fm, rays, starts)
        exits = np.full(len(rays), G.NONE, dtype=np.uint32)
        _FLAT["case"] = (fm, rays, G.seg_to_torch(ref), torch.from_numpy(exits))
    return _FLAT["case"]


def test_direction_gradient_is_orthogonal_to_the_direction_and_scales_inversely(foam_factory):
    """dt/dD has no component along D, and t does not depend on |D|: scaling D by 3 leaves the origin gradient as it
    is and divides the direction gradient by 3.  On rays whose directions are not unit (|D| between 0.3 and 7).  The
    dot product of a row with D is a sum of three products that cancel: it is held to 1e-12 of |row| |D| (float64
    rounds at 1.1e-16 and the row is itself a sum of about 25 cancelling terms; measured 4.1e-15)."""
    fm, rays, seg, exits = _flat(foam_factory)
    length = np.linalg.norm(rays[:, 3:], axis=1)
    assert length.min() < 0.9 and length.max() > 1.5
    rng = np.random.default_rng(21)
    total = seg["cells"].numel()
    g_enter, g_exit = torch.from_numpy(rng.normal(size=total)), torch.from_numpy(rng.normal(size=total))
    points = torch.from_numpy(fm["points"]).double()
    r = torch.from_numpy(rays).double()
    got = segment_rays_grad(seg, exits, points, r, g_enter, g_exit)
    assert bool(torch.isfinite(got).all()) and bool((got != 0).any(dim=1).all())
    along = (got[:, 3:] * r[:, 3:]).sum(-1).abs()
    scale = got[:, 3:].norm(dim=1) * r[:, 3:].norm(dim=1)
    print("largest |grad_D . D| / (|grad_D| |D|): %.3g" % float((along / scale).max()))
    assert bool((along <= 1e-12 * scale).all())

    scaled = r.clone()
    scaled[:, 3:] *= 3.0
    again = segment_rays_grad(seg, exits, points, scaled, g_enter, g_exit)
    torch.testing.assert_close(again[:, :3], got[:, :3], rtol=1e-9, atol=1e-12 * float(got[:, :3].abs().max()))
    torch.testing.assert_close(again[:, 3:] * 3.0, got[:, 3:], rtol=1e-9, atol=1e-12 * float(got[:, 3:].abs().max()))


def test_holder_rule(foam_factory):
    """The construction of tests/test_segments_grad.py::test_holder_rule: a gradient on t_enter alone gives exactly what
    the same values give as a gradient on t_exit, placed at the entry that holds each t_enter."""
    fm, rays, ref, exits = _case(foam_factory, max_intersections=20)
    seg = G.seg_to_torch(ref)
    held_by = G.holders_by_loop(ref["offsets"], ref["t_exit"])
    holder = ref["t_exit"] > ref["t_enter"]
    assert (~holder).sum() >= 5
    for dtype in (torch.float64, torch.float32):
        points = torch.from_numpy(fm["points"]).to(dtype)
        g = torch.from_numpy(np.random.default_rng(8).normal(size=len(holder))).to(dtype)
        zero = torch.zeros_like(g)
        held = torch.from_numpy(held_by >= 0)
        placed = torch.zeros_like(g).index_add(0, torch.from_numpy(held_by[held_by >= 0]), g[held])
        args = (seg, torch.from_numpy(exits), points, torch.from_numpy(rays))
        a = segment_rays_grad(*args, g, zero)
        b = segment_rays_grad(*args, zero, placed)
        assert a.dtype == dtype and a.shape == (len(ref["counts"]), 6) and bool((a != 0).any())
        assert torch.equal(a, b)


def test_hand_built_case():
    """Sites at (0,0,0) and (2,0,0), one ray from (-1,0,0) with D = (3,0,4): n = (2,0,0), num = 4, |D| = 5,
    d = (0.6, 0, 0.8), dp = 1.2 and t = 2 |D| / D_x = 10/3.  By hand dt/dO = -n / dp = (-5/3, 0, 0) and, from
    t = 2 |D| / D_x, dt/dD = (2/5 - 10/9, 0, 8/15)."""
    points = torch.tensor([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [9.0, 9.0, 9.0]], dtype=torch.float64)
    rays = torch.tensor([[-1.0, 0.0, 0.0, 3.0, 0.0, 4.0]], dtype=torch.float64)
    seg = {"offsets": torch.tensor([0, 1]), "cells": torch.tensor([0], dtype=torch.int32).to(torch.uint32),
           "t_enter": torch.tensor([0.0]), "t_exit": torch.tensor([10.0 / 3.0])}
    exits = torch.tensor([1], dtype=torch.int32).to(torch.uint32)
    e0, x0 = 0.3, 0.9
    g_enter, g_exit = torch.tensor([e0], dtype=torch.float64), torch.tensor([x0], dtype=torch.float64)
    got = segment_rays_grad(seg, exits, points, rays, g_enter, g_exit)
    want = x0 * torch.tensor([[-5.0 / 3.0, 0.0, 0.0, 2.0 / 5.0 - 10.0 / 9.0, 0.0, 8.0 / 15.0]], dtype=torch.float64)
    torch.testing.assert_close(got, want, rtol=1e-14, atol=1e-16)        # e0 belongs to t_enter = 0, a constant
    # the rays' leading shape does not matter, and float32 points give a float32 result
    got32 = segment_rays_grad(seg, exits, points.float(), rays.reshape(1, 1, 6), g_enter, g_exit)
    assert got32.dtype == torch.float32 and got32.shape == (1, 6)
    torch.testing.assert_close(got32.double(), want, rtol=1e-6, atol=1e-7)
    # without a cell behind the face it adds nothing
    none = torch.tensor([-1], dtype=torch.int32).view(torch.uint32)
    assert bool((segment_rays_grad(seg, none, points, rays, g_enter, g_exit) == 0).all())
    # nor does a face whose exit is infinite
    inf_seg = {**seg, "t_exit": torch.tensor([INF])}
    assert bool((segment_rays_grad(inf_seg, exits, points, rays, g_enter, g_exit) == 0).all())
    # a second ray without entries has a row of zeros
    two = {**seg, "offsets": torch.tensor([0, 1, 1])}
    got = segment_rays_grad(two, torch.cat([exits, none]), points, torch.cat([rays, rays]), g_enter, g_exit)
    torch.testing.assert_close(got[:1], want, rtol=1e-14, atol=1e-16)
    assert bool((got[1] == 0).all())


def test_zero_and_infinite_entries_add_nothing(foam_factory):
    """On the default-settings frame every ray ends in a cell without an exit: gradients on those entries alone give
    zeros.  A face parallel to the ray (dp = 0) with G == 0 exactly is skipped; with a gradient on it the ray's row is
    not finite, and only that ray's."""
    fm, rays, ref, exits = _case(foam_factory)
    assert (exits == G.NONE).all()
    seg = G.seg_to_torch(ref)
    points = torch.from_numpy(fm["points"])
    g = torch.where(torch.isinf(seg["t_exit"]), torch.ones_like(seg["t_exit"]), torch.zeros_like(seg["t_exit"]))
    assert int(g.sum()) == len(ref["counts"])
    got = segment_rays_grad(seg, torch.from_numpy(exits), points, torch.from_numpy(rays), torch.zeros_like(g), g)
    assert got.shape == (len(ref["counts"]), 6) and bool((got == 0).all())

    # ray 0: two faces, the first parallel to the ray (sites 0 and 1 differ in y only, the ray runs along x); ray 1: one
    points = torch.tensor([[0.0, 0.0, 0.0], [0.0, 2.0, 0.0], [3.0, 2.0, 0.0]], dtype=torch.float64)
    rays = torch.tensor([[-1.0, 0.5, 0.0, 1.0, 0.0, 0.0], [-1.0, 2.5, 0.0, 2.0, 0.0, 0.0]], dtype=torch.float64)
    seg = {"offsets": torch.tensor([0, 3, 5]),
           "cells": torch.tensor([0, 1, 2, 1, 2], dtype=torch.int32).to(torch.uint32),
           "t_enter": torch.tensor([0.0, 1.0, 2.5, 0.0, 2.5]), "t_exit": torch.tensor([1.0, 2.5, INF, 2.5, INF])}
    none = torch.tensor([-1, -1], dtype=torch.int32).view(torch.uint32)
    zero = torch.zeros(5, dtype=torch.float64)
    got = segment_rays_grad(seg, none, points, rays, zero, torch.tensor([0.0, 1.0, 5.0, 1.0, 5.0], dtype=torch.float64))
    assert bool(torch.isfinite(got).all())
    # face x = 1.5 between sites 1 and 2: n = (3,0,0), dp = 3, dt/dO = (-1,0,0); t = 2.5 |D| / D_x: nothing along x
    torch.testing.assert_close(got[:, :3], torch.tensor([[-1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]], dtype=torch.float64))
    assert bool((got[:, 3] == 0).all())
    got = segment_rays_grad(seg, none, points, rays, zero, torch.tensor([1.0, 1.0, 0.0, 1.0, 0.0], dtype=torch.float64))
    assert not bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())


def test_autograd_function_on_the_cpu(foam_factory):
    """The autograd function of Pipeline.trace_differentiable_segments, called directly (the pipeline needs a GPU): with
    rays that require grad rays.grad is segment_rays_grad's in the rays' own shape, points.grad is unchanged by it, and
    without it the backward returns None for the rays."""
    from radfoam_amd.segments import _SegmentTimes

    fm, rays, ref, exits = _case(foam_factory, weight_threshold=0.5)
    seg = G.seg_to_torch(ref)
    exits = torch.from_numpy(exits)
    rng = np.random.default_rng(9)
    density = torch.from_numpy(fm["attributes"][:, -1].astype(np.float64)) + 0.2
    rgb = torch.from_numpy(rng.uniform(0.0, 1.0, size=(density.numel(), 3)))
    points = torch.from_numpy(fm["points"])
    t_enter, t_exit = seg["t_enter"].clone().requires_grad_(True), seg["t_exit"].clone().requires_grad_(True)
    composite_segments({**seg, "t_enter": t_enter, "t_exit": t_exit}, density, rgb).sum().backward()
    want_rays = segment_rays_grad(seg, exits, points, torch.from_numpy(rays), t_enter.grad, t_exit.grad)
    want_points = segment_points_grad(seg, exits, points, torch.from_numpy(rays), t_enter.grad, t_exit.grad)
    assert bool(torch.isfinite(want_rays).all()) and bool((want_rays != 0).any())

    def run(points_grad, rays_grad):
        p = points.clone().requires_grad_(points_grad)
        r = torch.from_numpy(rays).reshape(48, 64, 6).clone().requires_grad_(rays_grad)
        te, tx = _SegmentTimes.apply(p, r.reshape(-1, 6), seg["offsets"], seg["cells"], exits, seg["t_enter"],
                                     seg["t_exit"])
        assert torch.equal(te, seg["t_enter"]) and torch.equal(tx, seg["t_exit"])
        composite_segments({**seg, "t_enter": te, "t_exit": tx}, density, rgb).sum().backward()
        return p.grad, r.grad

    p_grad, r_grad = run(True, True)
    assert r_grad.shape == (48, 64, 6) and r_grad.dtype == torch.float32
    assert torch.equal(r_grad.reshape(-1, 6), want_rays) and torch.equal(p_grad, want_points)
    p_grad, r_grad = run(False, True)
    assert p_grad is None and torch.equal(r_grad.reshape(-1, 6), want_rays)
    p_grad, r_grad = run(True, False)
    assert r_grad is None and torch.equal(p_grad, want_points)

    class Ctx:
        needs_input_grad = (True, False) + (False,) * 5
        saved_tensors = (points, torch.from_numpy(rays), seg["offsets"], seg["cells"], exits, seg["t_enter"],
                         seg["t_exit"])

    out = _SegmentTimes.backward(Ctx, t_enter.grad, t_exit.grad)
    assert out[1] is None and torch.equal(out[0], want_points) and all(o is None for o in out[2:])


def test_exported_names():
    import radfoam_amd

    assert radfoam.segment_rays_grad is radfoam_amd.segment_rays_grad
    assert "segment_rays_grad" in radfoam_amd.__all__


def test_example_drops_only_the_rays_whose_gradient_is_not_finite():
    """examples/fit_camera_pose.py hangs finite_rows on the rays: a ray whose row of the gradient is not finite leaves
    the step alone, and the pose gradient is the sum over all the other rays, not zero."""
    from examples.fit_camera_pose import finite_rows, pose_rays

    rng = np.random.default_rng(3)
    position = torch.from_numpy(rng.normal(size=3))
    directions = torch.from_numpy(rng.normal(size=(4, 5, 3)))
    upstream = torch.from_numpy(rng.normal(size=(4, 5, 6)))
    bad = upstream.clone()
    bad[1, 2, 4], bad[3, 0, 0], bad[3, 0, 5] = INF, float("nan"), -INF
    kept = upstream.clone()
    kept[1, 2], kept[3, 0] = 0.0, 0.0

    def pose_grad(weights, hook):
        pose = torch.tensor([0.3, -0.2, 0.1, 0.5, 0.4, -0.6], dtype=torch.float64, requires_grad=True)
        rays = pose_rays(pose, position, directions)
        if hook:
            rays.register_hook(finite_rows)
        (rays * weights).sum().backward()
        return pose.grad

    assert torch.equal(finite_rows(bad), kept) and torch.equal(finite_rows(upstream), upstream)
    assert not bool(torch.isfinite(pose_grad(bad, False)).all())
    got = pose_grad(bad, True)
    assert bool(torch.isfinite(got).all()) and bool((got != 0).all()) and torch.equal(got, pose_grad(kept, False))
