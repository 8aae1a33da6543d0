"""-m gpu: the epoch flush of the image backward (backward_replay_cached_kernel, backward_mode 3) against the CPU oracle.

The block's LDS gradient table is flushed between the two barriers of every epoch: rows that only ever received a
density gradient ("narrow") are sent by their owning thread, rows that received colour or point gradients ("wide") by
the whole wave, the rows are dealt to the four waves, and the block learns through a flag word whether any lane is still
alive.  Each case below is one way that can go wrong.  5,000-point foams, frames of at most 80x56 rays, the trail of a
forward on the same pipeline.  The bars are the project's: forward rgba bit-equal to the oracle, gradients
helpers.grad_close (1e-3 per element) and relative L2 below 1e-5.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_CASES = {}


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _case(foam_factory, d, seed, width, height, density=None, **settings):
    """Foam, frame, upstream gradient and the oracle's answers (one thread), computed once and never modified.
    density: None = as the factory gives it (zero shell, lit core), "zero" = every cell 0, "lit" = max(density, 4.5e-6)."""
    key = (d, seed, width, height, density, tuple(sorted(settings.items())))
    if key not in _CASES:
        fm = dict(foam_factory(5000, d, seed))
        if density is not None:
            fm["attributes"] = fm["attributes"].copy()
            dens = fm["attributes"][:, -1]
            fm["attributes"][:, -1] = 0.0 if density == "zero" else np.maximum(dens, np.float32(4.5e-6))
        cam, rays, start = H.camera_setup(fm, width, height)
        starts = np.full(rays.shape[:-1], start, dtype=np.uint32)
        g = np.random.default_rng(seed).normal(size=rays.shape[:-1] + (4,)).astype(np.float32)
        args = (d, fm["points"], fm["attributes"], fm["point_adjacency"], fm["point_adjacency_offsets"])
        fwd = O.trace_forward(*args, rays, starts, num_threads=1, **settings)
        bwd = O.trace_backward(*args, rays, starts, fwd["rgba"], g, num_threads=1, **settings)
        _CASES[key] = dict(d=d, fm=fm, rays=rays, starts=starts, g=g, fwd=fwd, bwd=bwd)
    return _CASES[key]


def _run(c, trail_steps=None, **settings):
    """Forward (records the trail) and cached image backward on one fp32 pipeline; the forward is checked bit for bit."""
    import radfoam

    pipe = radfoam.create_pipeline(c["d"])
    pipe.record_trail = True
    pipe.backward_mode = 3
    if trail_steps is not None:
        pipe.trail_steps = trail_steps
    p, a, adj, off = H.to_torch_foam(c["fm"], DEV)
    tr, ts = _t(c["rays"]), _t(c["starts"])
    f = pipe.trace_forward(p, a, adj, off, tr, ts, **settings)
    np.testing.assert_array_equal(f["rgba"].cpu().numpy().view(np.uint32), c["fwd"]["rgba"].view(np.uint32))
    assert pipe._trail is not None
    out = pipe.trace_backward(p, a, adj, off, tr, ts, f["rgba"], _t(c["g"]), **settings)
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy() for k in ("points_grad", "attr_grad")}


def _check(got, ref, what=""):
    for key in ("points_grad", "attr_grad"):
        ok, rel, worst = H.grad_close(got[key], ref[key])
        assert ok and rel < 1e-5, (what, key, rel, worst)
        assert np.abs(ref[key]).max() > 0


def _assert_a_narrow_row_turns_wide(c):
    """Input condition of the mixed cases: a cell of density exactly 0 with a point gradient (an empty `prev` cell at
    the lit boundary): its row collects density-only adds, then point gradients."""
    empty = c["fm"]["attributes"][:, -1].astype(np.float32) == 0.0
    moved = np.abs(c["bwd"]["points_grad"]).max(axis=1) != 0.0
    assert empty.any() and (~empty).any() and (empty & moved).any()


@pytest.mark.parametrize("d", [0, 1, 2, 3])
def test_mixed_rows(foam_factory, d):
    """Zero shell, lit core: narrow and wide rows share the table, and rows turn wide after density-only adds.  The
    frame's height is not a multiple of the 16-row tile."""
    c = _case(foam_factory, d, 70 + d, 80, 56)
    _assert_a_narrow_row_turns_wide(c)
    _check(_run(c), c["bwd"], d)


def test_mixed_rows_half(foam_factory):
    """The fp16 instance of the same: fp16 attributes and upstream gradient, fp32 accumulators (dense rows) against the
    oracle's fp32 mode on the widened values, the forward bit-equal to the oracle's fp16 mode."""
    import radfoam

    d = 2
    key = ("half", d)
    if key not in _CASES:
        _CASES[key] = H.half_backward_case(foam_factory, d, 70 + d, True, False, False)
    c = _CASES[key]
    _assert_a_narrow_row_turns_wide(dict(fm=c["fm"], bwd=c["bwd32"]))
    pipe = radfoam.create_pipeline(d, torch.float16)
    pipe.record_trail = True
    pipe.backward_mode = 3
    pipe.gradient_row_pitch = "dense"
    p, a, adj, off = H.to_torch_foam(c["fm"], DEV)
    assert a.dtype == torch.float16
    tr, ts = _t(c["rays"]), _t(c["starts"])
    f = pipe.trace_forward(p, a, adj, off, tr, ts)
    np.testing.assert_array_equal(f["rgba"].cpu().numpy().view(np.uint16), c["fwd"]["rgba"].view(np.uint16))
    out = pipe.trace_backward(p, a, adj, off, tr, ts, _t(c["fwd"]["rgba"]), _t(c["g"]))
    torch.cuda.synchronize()
    n, A = c["fm"]["attributes"].shape
    acc = out["flat_grad"][-n * A:].view(n, A)
    assert acc.dtype == torch.float32
    _check({"points_grad": out["points_grad"].cpu().numpy(), "attr_grad": acc.cpu().numpy()}, c["bwd32"], "fp16")


def test_every_cell_empty(foam_factory):
    """Density 0 everywhere: only narrow rows exist.  The density column matches the oracle; every other column and
    all of points_grad are exactly zero (a wrong column or a stale mark would show here)."""
    d = 2
    c = _case(foam_factory, d, 75, 80, 56, density="zero")
    ref = c["bwd"]
    assert float(c["fwd"]["rgba"].max()) == 0.0 and np.abs(ref["attr_grad"][:, -1]).max() > 0
    assert not ref["attr_grad"][:, :-1].any() and not ref["points_grad"].any()
    got = _run(c)
    ok, rel, worst = H.grad_close(got["attr_grad"][:, -1], ref["attr_grad"][:, -1])
    assert ok and rel < 1e-5, (rel, worst)
    assert not got["attr_grad"][:, :-1].any()
    assert not got["points_grad"].any()


@pytest.mark.parametrize("d", [2, 3])
def test_every_segment_lit(foam_factory, d):
    """density = max(density, 4.5e-6): every row is wide, so every eviction goes through the cooperative loop and the
    dealt ownership (160 rows at degree 2, 124 at degree 3)."""
    c = _case(foam_factory, d, 76 + d, 80, 56, density="lit")
    assert (c["fm"]["attributes"][:, -1] > 0).all()
    _check(_run(c), c["bwd"], d)


@pytest.mark.parametrize("side", [16, 17])
def test_one_block_and_nearly_empty_blocks(foam_factory, side):
    """16x16: one full block.  17x17: four blocks, three of them with 17, 17 and 1 rays, so whole waves without a ray
    go through every epoch's flag and barriers."""
    c = _case(foam_factory, 2, 80, side, side)
    _check(_run(c), c["bwd"], side)


def test_no_ray_fits_the_trail(foam_factory):
    """trail_steps = 5 with every ray longer: every lane is dead from the start, the first epoch ends the block with a
    full flush of an empty table, and the re-walk launch supplies the gradients."""
    c = _case(foam_factory, 2, 81, 80, 56)
    assert int(c["fwd"]["num_intersections"].min()) > 5
    _check(_run(c, trail_steps=5), c["bwd"])


@pytest.mark.parametrize("settings", [dict(weight_threshold=0.0), dict(max_intersections=3),
                                      dict(weight_threshold=0.0, max_intersections=3)],
                         ids=["threshold0", "max3", "threshold0-max3"])
def test_rays_that_end_inside_an_epoch(foam_factory, settings):
    """weight_threshold = 0 (rays run until they leave the foam, each after its own number of steps) and
    max_intersections = 3 (rays stop before the first epoch ends): waves finish at different times."""
    c = _case(foam_factory, 2, 82, 80, 56, **settings)
    for key in ("points_grad", "attr_grad"):
        assert np.isfinite(c["bwd"][key]).all()
    _check(_run(c, **settings), c["bwd"], settings)
