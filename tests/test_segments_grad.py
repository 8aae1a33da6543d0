"""CPU: radfoam.segment_points_grad (the vectorised torch restatement of DESIGN 4.9) on segments of the CPU oracle
(oracle.trace_paths; the 64x48 frame of foam_factory(3000, 2, 21) under the default settings, weight_threshold = 0.5 and
max_intersections = 20): finite differences, the holder rule, the cells behind the last faces, a case small enough to
do by hand, and the entries that must add nothing."""
import numpy as np
import torch

import radfoam
from radfoam import composite_segments, segment_points_grad
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


def test_finite_differences(foam_factory):
    """Every 8th ray of the weight_threshold = 0.5 frame (384 rays; finite and infinite last exits, a non-holder entry
    among them).  The function differentiated is float64 throughout: the times of the FIXED cell sequence from the exact
    bisectors (segments_grad_ref.exact_times, holders as the stored floats decide them), composited by
    composite_segments with the foam's density + 0.2 and a random colour, weighted by random numbers and summed.  Its
    gradient by the restatement (autograd through composite_segments down to the times, segment_points_grad from there)
    is compared on 50 coordinates -- the start cell, a cell that is only ever an exit cell, 48 random ones of the cells
    the rays touch -- with central differences.

    The step is the one of 2^-16 .. 2^-23 at which halving it changes the estimates least (largest change over the 50).
    A central difference at step h is off by c h^2 plus round-off / h; in the h^2 regime the change on halving is 3/4
    of the error at h, and at the turning point the round-off of the two estimates adds as much again: the bar is twice
    the change.  Measured: step 2^-21 = 4.8e-7, change on halving 7.4e-7 (8.5e-5 at 2^-17, 6.9e-6 at 2^-23), difference
    to the restatement 3.9e-7, on gradients of up to 343."""
    fm, rays, ref, exits = _case(foam_factory, weight_threshold=0.5)
    seg, exits, rays = _subset(ref, exits, rays, np.arange(0, len(ref["counts"]), 8))
    held_by = G.holders_by_loop(seg["offsets"].numpy(), seg["t_exit"].numpy())
    after = G.next_cells(seg, exits)
    last = seg["t_exit"][seg["offsets"][1:] - 1]
    assert torch.isfinite(last).any() and torch.isinf(last).any()
    assert (seg["t_exit"] <= seg["t_enter"]).any()

    rng = np.random.default_rng(7)
    points = torch.from_numpy(fm["points"]).double()
    density = torch.from_numpy(fm["attributes"][:, -1].astype(np.float64)) + 0.2    # no empty cells: every face counts
    rgb = torch.from_numpy(rng.uniform(0.0, 1.0, size=(density.numel(), 3)))
    weights = torch.from_numpy(rng.normal(size=(len(rays), 4)))

    def loss_at(t_enter, t_exit):
        return (composite_segments({**seg, "t_enter": t_enter, "t_exit": t_exit}, density, rgb) * weights).sum()

    t_enter, t_exit = (t.requires_grad_(True) for t in G.exact_times(points, rays, seg, after, held_by))
    loss_at(t_enter, t_exit).backward()
    got = segment_points_grad(seg, torch.from_numpy(exits), points, torch.from_numpy(rays), t_enter.grad, t_exit.grad)
    assert got.dtype == torch.float64 and got.shape == points.shape and bool(torch.isfinite(got).all())

    cells = seg["cells"].numpy()
    only_exit = np.setdiff1d(exits[exits != G.NONE], cells)
    assert only_exit.size
    coords = [(int(cells[0]), 2), (int(only_exit[0]), 0)]
    coords += [(int(c), int(a)) for c, a in zip(rng.choice(np.unique(cells), 48, replace=False), rng.integers(0, 3, 48))]
    want = np.array([float(got[c, a]) for c, a in coords])
    assert np.abs(want).max() > 1.0 and (want != 0).sum() >= 45

    def central(h):
        out = []
        for c, a in coords:
            moved = []
            for sign in (1.0, -1.0):
                p = points.clone()
                p[c, a] += sign * h
                moved.append(float(loss_at(*G.exact_times(p, rays, seg, after, held_by))))
            out.append((moved[0] - moved[1]) / (2.0 * h))
        return np.array(out)

    steps = [2.0 ** -k for k in range(16, 25)]
    estimates = [central(h) for h in steps]
    change = [float(np.abs(a - b).max()) for a, b in zip(estimates[:-1], estimates[1:])]
    best = int(np.argmin(change))
    print("change on halving, step by step:", ["%.2g" % c for c in change])
    error = float(np.abs(estimates[best] - want).max())
    print("step %.3g: change on halving %.3g, difference to the restatement %.3g, largest gradient %.3g"
          % (steps[best], change[best], error, np.abs(want).max()))
    assert change[best] < 1e-5 * np.abs(want).max()
    assert error <= 2.0 * change[best]


def test_holder_rule(foam_factory):
    """A gradient on t_enter alone gives exactly what the same values give as a gradient on t_exit, placed at the entry
    that holds each t_enter (found by the walk's own loop t0 = max(t0, t1)); those in front of a ray's first holder
    are dropped."""
    fm, rays, ref, exits = _case(foam_factory, max_intersections=20)
    seg = G.seg_to_torch(ref)
    held_by = G.holders_by_loop(ref["offsets"], ref["t_exit"])
    holder = ref["t_exit"] > ref["t_enter"]
    assert (~holder).sum() >= 5                                  # zero-length crossings: t_enter skips over them
    follows_non_holder = np.flatnonzero(~holder[:-1]) + 1
    assert (held_by[follows_non_holder] != follows_non_holder - 1).all()
    assert (held_by == -1).sum() >= len(ref["counts"])           # every ray's first entry at least
    for dtype in (torch.float64, torch.float32):
        points = torch.from_numpy(fm["points"]).to(dtype)
        g = torch.from_numpy(np.random.default_rng(8).normal(size=len(holder))).to(dtype)
        zero = torch.zeros_like(g)
        placed = torch.zeros_like(g).index_add(0, torch.from_numpy(held_by[held_by >= 0]), g[torch.from_numpy(held_by >= 0)])
        args = (seg, torch.from_numpy(exits), points, torch.from_numpy(rays))
        a = segment_points_grad(*args, g, zero)
        b = segment_points_grad(*args, zero, placed)
        assert a.dtype == dtype and bool((a != 0).any())
        assert torch.equal(a, b)


def _scan_winner(fm, cell, ray):
    """The neighbour behind the face the reference's scan picks for `ray` in `cell`: the fp16 offsets of the face table,
    the smallest t = ((P + o/2) - O) . o / (o . d) among the faces with o . d > 0 (float64 here)."""
    off, adj = fm["point_adjacency_offsets"], fm["point_adjacency"]
    nbrs = adj[off[cell]:off[cell + 1]].astype(np.int64)
    p = fm["points"][cell].astype(np.float64)
    o = (fm["points"][nbrs] - fm["points"][cell]).astype(np.float16).astype(np.float64)
    d = ray[3:].astype(np.float64) / np.linalg.norm(ray[3:].astype(np.float64))
    dp = o @ d
    t = np.where(dp > 0, ((p + o / 2 - ray[:3].astype(np.float64)) * o).sum(-1) / np.where(dp > 0, dp, 1.0), np.inf)
    return int(nbrs[np.argmin(t)]), float(t.min())


def test_exit_cells_are_the_longer_walks_next_entries(foam_factory):
    """What rf_trace_segments_exit_cells computes -- scan the last entry's cell once more, follow the winner -- is, for a
    walk cut short by the threshold or the step limit, the entry at the same position of the default-settings walk of
    the same ray.  Both kinds of ending occur in both cases."""
    for settings in ({"weight_threshold": 0.5}, {"max_intersections": 20}):
        fm, rays, ref, exits = _case(foam_factory, **settings)
        has = ref["counts"] > 0
        last = ref["offsets"][1:][has] - 1
        finite = np.isfinite(ref["t_exit"][last])
        assert finite.any() and (~finite).any() and has.all()
        assert ((exits != G.NONE) == finite).all()
        for r in np.flatnonzero(finite):
            winner, t = _scan_winner(fm, int(ref["cells"][last[r]]), rays[r])
            assert winner == int(exits[r])
            assert abs(t - float(ref["t_exit"][last[r]])) <= 1e-5 * max(1.0, abs(t))


def test_hand_built_case():
    """Sites at x = 0, 2, 5 on the x axis, one ray from (-1, 0, 0) along it (direction not normalised).  The faces are
    x = 1 (t = 2) and x = 3.5 (t = 4.5), and t = (p_a + p_b) / 2 - O along x, so dt/dp_a = dt/dp_b = (1/2, 0, 0).  The
    walk is cut after two entries: the second has a finite exit and the third site is known as exit_cells only."""
    points = torch.tensor([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [5.0, 0.0, 0.0], [9.0, 9.0, 9.0]], dtype=torch.float64)
    rays = torch.tensor([[-1.0, 0.0, 0.0, 3.0, 0.0, 0.0]])
    seg = {"offsets": torch.tensor([0, 2]), "cells": torch.tensor([0, 1], dtype=torch.int32).to(torch.uint32),
           "t_enter": torch.tensor([0.0, 2.0]), "t_exit": torch.tensor([2.0, 4.5])}
    e0, e1, x0, x1 = 0.3, -1.7, 0.9, 2.2
    g_enter, g_exit = torch.tensor([e0, e1], dtype=torch.float64), torch.tensor([x0, x1], dtype=torch.float64)
    exits = torch.tensor([2], dtype=torch.int32).to(torch.uint32)
    got = segment_points_grad(seg, exits, points, rays, g_enter, g_exit)
    g0, g1 = x0 + e1, x1                     # e0 belongs to t_enter = 0, a constant
    want = torch.zeros(4, 3, dtype=torch.float64)
    want[0, 0], want[1, 0], want[2, 0] = 0.5 * g0, 0.5 * g0 + 0.5 * g1, 0.5 * g1
    torch.testing.assert_close(got, want, rtol=1e-15, atol=0.0)
    # without a cell behind the last face, that face adds nothing on either side
    none = torch.tensor([-1], dtype=torch.int32).view(torch.uint32)
    got = segment_points_grad(seg, none, points, rays, g_enter, g_exit)
    want[1, 0], want[2, 0] = 0.5 * g0, 0.0
    torch.testing.assert_close(got, want, rtol=1e-15, atol=0.0)
    # float32 points give a float32 result
    got32 = segment_points_grad(seg, exits, points.float(), rays, g_enter, g_exit)
    assert got32.dtype == torch.float32


def test_zero_and_infinite_entries_add_nothing(foam_factory):
    """Entries whose t_exit is infinite have no face; faces whose total G is exactly 0 are skipped even where their
    derivative is not finite (a face parallel to the ray: dp = 0)."""
    fm, rays, ref, exits = _case(foam_factory)
    assert (exits == G.NONE).all()
    seg = G.seg_to_torch(ref)
    points = torch.from_numpy(fm["points"])
    g = torch.where(torch.isinf(seg["t_exit"]), torch.ones_like(seg["t_exit"]), torch.zeros_like(seg["t_exit"]))
    assert int(g.sum()) == len(ref["counts"])
    got = segment_points_grad(seg, torch.from_numpy(exits), points, torch.from_numpy(rays), torch.zeros_like(g), g)
    assert bool((got == 0).all())

    # two faces: the first parallel to the ray (sites 0 and 1 differ in y only, the ray runs along x), the second not
    points = torch.tensor([[0.0, 0.0, 0.0], [0.0, 2.0, 0.0], [3.0, 2.0, 0.0]], dtype=torch.float64)
    rays = torch.tensor([[-1.0, 0.5, 0.0, 1.0, 0.0, 0.0]])
    seg = {"offsets": torch.tensor([0, 3]), "cells": torch.tensor([0, 1, 2], dtype=torch.int32).to(torch.uint32),
           "t_enter": torch.tensor([0.0, 1.0, 2.5]), "t_exit": torch.tensor([1.0, 2.5, INF])}
    none = torch.tensor([-1], dtype=torch.int32).view(torch.uint32)
    zero = torch.zeros(3, dtype=torch.float64)
    got = segment_points_grad(seg, none, points, rays, zero, torch.tensor([0.0, 1.0, 5.0], dtype=torch.float64))
    assert bool(torch.isfinite(got).all()) and bool((got[0] == 0).all())
    torch.testing.assert_close(got[1:, 0], torch.tensor([0.5, 0.5], dtype=torch.float64), rtol=1e-15, atol=0.0)
    # ... and with a gradient on the parallel face the result is not finite: no guard beyond bisector_grad's
    got = segment_points_grad(seg, none, points, rays, zero, torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64))
    assert not bool(torch.isfinite(got[:2]).all())


def test_composition_with_infinite_last_exits(foam_factory):
    """composite_segments over t_enter / t_exit that require grad, on a frame whose every ray ends in a cell without an
    exit (t_exit = inf): finite gradients down to the times and down to the points, through the autograd function
    Pipeline.trace_differentiable_segments uses as well."""
    from radfoam_amd.segments import _SegmentTimes

    fm, rays, ref, exits = _case(foam_factory)
    seg = G.seg_to_torch(ref)
    assert np.isinf(ref["t_exit"][ref["offsets"][1:] - 1]).all()
    rng = np.random.default_rng(9)
    density = torch.from_numpy(fm["attributes"][:, -1].astype(np.float64))
    rgb = torch.from_numpy(rng.uniform(0.0, 1.0, size=(density.numel(), 3)))
    t_enter, t_exit = seg["t_enter"].clone().requires_grad_(True), seg["t_exit"].clone().requires_grad_(True)
    composite_segments({**seg, "t_enter": t_enter, "t_exit": t_exit}, density, rgb).sum().backward()
    for g in (t_enter.grad, t_exit.grad):
        assert bool(torch.isfinite(g).all()) and bool((g != 0).any())
    points = torch.from_numpy(fm["points"])
    direct = segment_points_grad(seg, torch.from_numpy(exits), points, torch.from_numpy(rays), t_enter.grad, t_exit.grad)
    assert bool(torch.isfinite(direct).all()) and bool((direct != 0).any())

    p = points.clone().requires_grad_(True)
    te, tx = _SegmentTimes.apply(p, torch.from_numpy(rays), seg["offsets"], seg["cells"], torch.from_numpy(exits),
                                 seg["t_enter"], seg["t_exit"])
    assert torch.equal(te, seg["t_enter"]) and torch.equal(tx, seg["t_exit"])
    composite_segments({**seg, "t_enter": te, "t_exit": tx}, density, rgb).sum().backward()
    assert torch.equal(p.grad, direct)


def test_exported_names():
    import radfoam_amd

    assert radfoam.segment_points_grad is radfoam_amd.segment_points_grad
    assert callable(radfoam_amd.Pipeline.trace_differentiable_segments)
