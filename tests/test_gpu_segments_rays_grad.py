"""The kernel behind radfoam.segment_rays_grad on the GPU: against the float64 restatement of its
definition on the cases of tests/test_gpu_segments_grad.py, on hand-made lists that put runs of every length at every
lane position (the operator is defined on any CSR; the restatement on the same data is the truth), with lanes that must
be skipped, and through autograd from a composited loss down to rays.grad."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import segments_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _pipeline(d, dtype=torch.float32):
    import radfoam

    return radfoam.create_pipeline(d, dtype)


def _device_inputs(fm, rays, starts, attr_dtype=None):
    p, a, adj, off = H.to_torch_foam(fm, DEV, attr_dtype)
    r = torch.from_numpy(np.ascontiguousarray(rays)).to(DEV)
    s = torch.from_numpy(np.ascontiguousarray(starts, dtype=np.uint32)).to(DEV)
    return p, a, adj, off, r, s


_FLAT = {}


def _flat_case(foam_factory):
    """The flat case of tests/test_gpu_segments.py: 6000 points, 3000 incoherent un-normalised rays."""
    if not _FLAT:
        fm = foam_factory(6000, 0, 11)
        _FLAT["case"] = (fm,) + H.random_rays(fm, 3000, seed=3)
    return _FLAT["case"]


def _restatements(seg, exit_cells, points, rays, g_enter, g_exit):
    """The float64 and the float32 torch restatement on the device tensors the kernel gets."""
    import radfoam

    plain = {k: v.detach() for k, v in seg.items()}
    args = (rays.detach().reshape(-1, 6), g_enter, g_exit)
    ref64 = radfoam.segment_rays_grad(plain, exit_cells, points.detach().double(), *args, backend="torch")
    ref32 = radfoam.segment_rays_grad(plain, exit_cells, points.detach(), *args, backend="torch")
    assert ref64.dtype == torch.float64 and ref32.dtype == torch.float32 and ref64.is_cuda
    return ref64.cpu().numpy(), ref32.cpu().numpy()


def _assert_bars(name, got, ref64, ref32):
    """Per element helpers.grad_close at 1e-3 (the project's gradient bar).  Relative L2: 4 times the distance of the
    float32 restatement, and never less than 1e-6 = 16 fp32 roundings: the kernel sums in double and rounds once, so
    it is a rounding or two away, and on an easy case the float32 restatement may happen to be as close."""
    assert np.isfinite(ref64).all() and np.abs(ref64).max() > 0
    ok, rel, worst = H.grad_close(got, ref64)
    _, rel32, _ = H.grad_close(ref32, ref64)
    print("%s: relative L2 to the float64 restatement: kernel %.3g, float32 restatement %.3g; worst element at %.3g "
          "of its bound" % (name, rel, rel32, worst))
    assert ok, (name, worst)
    assert rel <= max(4.0 * rel32, 1e-6), (name, rel, rel32)


def _random_grads(total, seed=12):
    rng = np.random.default_rng(seed)
    return (torch.from_numpy(rng.normal(size=total).astype(np.float32)).to(DEV),
            torch.from_numpy(rng.normal(size=total).astype(np.float32)).to(DEV))


def _check(name, seg, exit_cells, points, rays, g_enter, g_exit):
    import radfoam

    num_rays = seg["offsets"].numel() - 1
    got = radfoam.segment_rays_grad(seg, exit_cells, points, rays, g_enter, g_exit)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and got.shape == (num_rays, 6) and got.is_cuda
    ref64, ref32 = _restatements(seg, exit_cells, points, rays, g_enter, g_exit)
    _assert_bars(name, got.cpu().numpy(), ref64, ref32)
    return got, ref64


_KERNEL_CASES = {
    "image": ("image", {}, None),
    "image_threshold": ("image", {"weight_threshold": 0.5}, None),
    "image_cap": ("image", {"max_intersections": 20}, None),
    "flat_3000": ("flat", {}, 3000),
    "flat_2999": ("flat", {}, 2999),
    "image_fp16": ("image16", {"weight_threshold": 0.5}, None),
}


def _traced(foam_factory, name):
    kind, kw, count = _KERNEL_CASES[name]
    if kind == "flat":
        fm, rays, starts = _flat_case(foam_factory)
        rays, starts = rays[:count], starts[:count]
        pipe, inputs = _pipeline(0), _device_inputs(fm, rays, starts)
    else:
        fm, rays, starts, _ = S.image_case(foam_factory)
        half = kind == "image16"
        pipe = _pipeline(2, torch.float16 if half else torch.float32)
        inputs = _device_inputs(fm, rays, starts, torch.float16 if half else None)
    return pipe, inputs, pipe.trace_differentiable_segments(*inputs, **kw)


@pytest.mark.parametrize("name", list(_KERNEL_CASES))
def test_kernel_against_float64_restatement(foam_factory, name):
    """Random normal gradients on every entry, as tests/test_gpu_segments_grad.py has them: the nearly grazing faces
    carry the rows they touch, and the kernel forms its contributions and its sums in double."""
    _, inputs, seg = _traced(foam_factory, name)
    total = seg["cells"].numel()
    last = seg["t_exit"][seg["offsets"][1:] - 1]
    assert bool(torch.isfinite(last).any()) or not _KERNEL_CASES[name][1]
    _check(name, seg, seg["exit_cells"], inputs[0], inputs[4], *_random_grads(total))


def _list_of(seg, keep=None):
    """The four arrays of a walk, detached, as a dict; `keep` (bool [S]) selects entries."""
    out = {k: seg[k].detach() for k in ("cells", "t_enter", "t_exit")}
    if keep is not None:
        out = {k: _take(v, keep) for k, v in out.items()}
    return out


def _take(t, index):
    """t[index] (uint32 tensors are indexed through their int32 view)."""
    if t.dtype == torch.uint32:
        return t.view(torch.int32)[index].contiguous().view(torch.uint32)
    return t[index].contiguous()


def test_long_rays_span_waves_and_blocks(foam_factory):
    """The image case's list under every 24th offset, with the ray rows at the same stride: 128 rays of about 600
    entries, each over several waves and blocks, so a ray's row is the sum of one update per wave it reaches into."""
    _, inputs, seg = _traced(foam_factory, "image")
    offsets = seg["offsets"][::24].contiguous()
    assert offsets.numel() == 129 and int(offsets[-1]) == seg["cells"].numel()
    counts = offsets[1:] - offsets[:-1]
    assert int(counts.min()) > 128 and int(counts.max()) < 1200
    long = {**_list_of(seg), "offsets": offsets}
    rays = inputs[4].reshape(-1, 6)[::24].contiguous()
    exits = seg["exit_cells"][23::24].contiguous()
    _check("long rays", long, exits, inputs[0], rays, *_random_grads(seg["cells"].numel()))


def test_many_rays_per_wave(foam_factory):
    """max_intersections = 2 on the flat rays, and the second entry of every third ray taken out: runs of 2, 2, 1 in
    turn, 38 rays to a wave, so that runs of either length begin at every lane (5 and 64 share no factor)."""
    fm, rays, starts = _flat_case(foam_factory)
    pipe, inputs = _pipeline(0), _device_inputs(fm, rays, starts)
    seg = pipe.trace_differentiable_segments(*inputs, max_intersections=2)
    offsets = seg["offsets"]
    counts = offsets[1:] - offsets[:-1]
    assert int(counts.min()) >= 1 and int(counts.max()) == 2 and int((counts == 2).sum()) > 2900
    drop = torch.zeros(seg["cells"].numel(), dtype=torch.bool, device=DEV)
    third = torch.arange(0, counts.numel(), 3, device=DEV)
    third = third[counts[third] == 2]
    drop[offsets[third] + 1] = True
    new_counts = counts.clone()
    new_counts[third] -= 1
    short = {**_list_of(seg, ~drop), "offsets": torch.cat([offsets[:1], torch.cumsum(new_counts, 0)])}
    first = short["offsets"][:-1] % 64
    for length in (1, 2):
        assert torch.unique(first[new_counts == length]).numel() == 64
    total = short["cells"].numel()
    _check("many rays per wave", short, seg["exit_cells"], inputs[0], inputs[4], *_random_grads(total))


def test_empty_rays_and_a_partial_last_wave(foam_factory):
    """The threshold frame's list with every fifth ray doubled by one without entries (a repeated offset) and the last
    3 entries dropped: rows of zeros between the others, and a last wave whose upper lanes have no entry."""
    _, inputs, seg = _traced(foam_factory, "image_threshold")
    total = seg["cells"].numel() - 3
    assert total % 64 != 0
    offsets = seg["offsets"].clamp_max(total)
    which = torch.arange(offsets.numel() - 1, device=DEV)
    repeat = torch.where(which % 5 == 0, 2, 1)
    source = torch.repeat_interleave(which, repeat)                        # the ray each new ray takes its row from
    ends = offsets[1:][source]                                             # the second copy ends where the first did
    holes = {**_list_of(seg, torch.arange(seg["cells"].numel(), device=DEV) < total),
             "offsets": torch.cat([offsets[:1], ends])}
    counts = holes["offsets"][1:] - holes["offsets"][:-1]
    assert int((counts == 0).sum()) >= 600 and bool((counts >= 0).all()) and int(holes["offsets"][-1]) == total
    rays = inputs[4].reshape(-1, 6)[source].contiguous()
    exits = _take(seg["exit_cells"], source)
    got, ref64 = _check("empty rays", holes, exits, inputs[0], rays, *_random_grads(total))
    assert bool((got[counts == 0] == 0).all())
    assert int((got[counts > 0] != 0).any(dim=1).sum()) > 0.9 * int((counts > 0).sum())


def test_skipped_lanes_leave_their_neighbours_alone(foam_factory):
    """Through the C entry point with an entry_ray of our own: entries whose entry_ray is out of range, or names a ray
    that does not own them, add nothing, and the sums of the runs they sit in, begin or end come out whole.  Such an
    entry still counts in the G of the holder in front of it (G is read from the lists by position), so the truth is the
    restatement with that entry's face taken away: its t_exit set to +inf, which changes no other face when the entry
    is a holder already (asserted).  Then upstream gradients that are exactly zero on every other ray: those rows are
    zero and the rows between them right."""
    from radfoam_amd import _lib
    from radfoam_amd.pipeline import _ptr, _stream_ptr

    _, inputs, seg = _traced(foam_factory, "image_threshold")
    points, rays = inputs[0], inputs[4].reshape(-1, 6).contiguous()
    offsets, total = seg["offsets"], seg["cells"].numel()
    num_rays = offsets.numel() - 1
    counts = offsets[1:] - offsets[:-1]
    entry_ray = torch.repeat_interleave(torch.arange(num_rays, dtype=torch.int32, device=DEV), counts,
                                        output_size=total)
    off = offsets.cpu().numpy()
    stored_exit = seg["t_exit"].detach().cpu().numpy()
    usable = (stored_exit > seg["t_enter"].detach().cpu().numpy()) & np.isfinite(stored_exit)   # holders with a face
    ray_of = np.searchsorted(off, np.arange(total), side="right") - 1
    usable &= (ray_of > 50) & (ray_of < num_rays - 1)            # so that rays 0, 40 and R - 1 below do not own them
    first, last = np.zeros(total, bool), np.zeros(total, bool)
    first[off[:-1]], last[off[1:] - 1] = True, True
    inner = usable & ~first & ~last
    lane = np.arange(total) % 64
    pair = int(np.flatnonzero(inner[:-1] & inner[1:] & (ray_of[:-1] == ray_of[1:]))[5])
    # a ray's first entry, a last one, a middle one, two in a row, lane 0 and lane 63 of a wave
    where = [int(np.flatnonzero(usable & first)[3]), int(np.flatnonzero(usable & last)[4]),
             int(np.flatnonzero(inner)[40]), pair, pair + 1, int(np.flatnonzero(usable & (lane == 0))[6]),
             int(np.flatnonzero(usable & (lane == 63))[7])]
    garbage = [-1, num_rays, 2 ** 31 - 1, num_rays + 5, 0, -2 ** 31, 40]
    assert len(set(where)) == len(where)
    for k, value in zip(where, garbage):
        entry_ray[k] = value

    def launch(g_enter, g_exit):
        out = torch.zeros((num_rays, 6), dtype=torch.float32, device=DEV)
        with torch.cuda.device(DEV):
            rc = _lib.load().rf_segments_rays_grad(
                points.size(0), _ptr(points), num_rays, _ptr(rays), _ptr(offsets), total, _ptr(entry_ray),
                _ptr(seg["cells"]), _ptr(seg["t_enter"].detach()), _ptr(seg["t_exit"].detach()),
                _ptr(seg["exit_cells"]), _ptr(g_enter), _ptr(g_exit), _ptr(out), _stream_ptr(torch.device(DEV)))
        _lib.check(rc)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    t_exit = seg["t_exit"].detach().clone()
    t_exit[torch.tensor(where, device=DEV)] = float("inf")
    without = {**_list_of(seg), "t_exit": t_exit, "offsets": offsets}
    g_enter, g_exit = _random_grads(total)
    ref64, ref32 = _restatements(without, seg["exit_cells"], points, rays, g_enter, g_exit)
    whole, _ = _restatements({**_list_of(seg), "offsets": offsets}, seg["exit_cells"], points, rays, g_enter, g_exit)
    # those faces did count (the restatement's index_add on the device is atomic: two runs differ by roundings)
    assert (np.abs(whole - ref64).max(axis=1) > 1e-9 * np.abs(whole).max()).sum() == len(set(ray_of[where]))
    _assert_bars("skipped lanes", launch(g_enter, g_exit), ref64, ref32)

    odd = torch.from_numpy(ray_of % 2 == 1).to(DEV)
    g_enter, g_exit = g_enter.masked_fill(odd, 0.0), g_exit.masked_fill(odd, 0.0)
    ref64, ref32 = _restatements(without, seg["exit_cells"], points, rays, g_enter, g_exit)
    got = launch(g_enter, g_exit)
    _assert_bars("every other ray zero", got, ref64, ref32)
    assert (got[1::2] == 0).all() and (got[0::2] != 0).any(axis=1).sum() > num_rays // 2 - 10


def test_autograd_end_to_end(foam_factory):
    """rays and points requiring grad together, loss.backward() through composite_segments (float64): rays.grad has the
    rays' shape and meets the bars against the restatement fed the same t gradients; points.grad is what the same call
    gives when the rays do not require grad (two runs of atomics: equal to the per-element bar, not bit for bit)."""
    import radfoam

    fm, rays, starts, _ = S.image_case(foam_factory)
    rng = np.random.default_rng(13)
    density = torch.from_numpy(fm["attributes"][:, -1].astype(np.float64) + 0.2).to(DEV)
    rgb = torch.from_numpy(rng.uniform(0.0, 1.0, size=(density.numel(), 3))).to(DEV)
    weights = torch.from_numpy(rng.normal(size=(48 * 64, 4))).to(DEV)
    pipe = _pipeline(2)

    def run(points_grad, rays_grad):
        p, a, adj, off, r, s = _device_inputs(fm, rays, starts)
        p.requires_grad_(points_grad)
        r.requires_grad_(rays_grad)
        seg = pipe.trace_differentiable_segments(p, a, adj, off, r, s, weight_threshold=0.5)
        return p, a, adj, off, r, s, seg

    p, a, adj, off, r, s, seg = run(True, True)
    assert seg["t_enter"].grad_fn is not None and seg["t_exit"].grad_fn is not None
    plain = pipe.trace_segments(p, a, adj, off, r, s, weight_threshold=0.5)
    assert sorted(seg) == sorted(list(plain) + ["exit_cells"])
    for k in plain:
        assert seg[k].dtype == plain[k].dtype and seg[k].shape == plain[k].shape
    for k in ("t_enter", "t_exit"):
        assert torch.equal(seg[k].detach().view(torch.int32), plain[k].view(torch.int32))
    (radfoam.composite_segments(seg, density, rgb) * weights).sum().backward()
    torch.cuda.synchronize()
    assert r.grad is not None and r.grad.shape == (48, 64, 6) and r.grad.dtype == torch.float32
    assert p.grad is not None and a.grad is None

    t_enter, t_exit = plain["t_enter"].clone().requires_grad_(True), plain["t_exit"].clone().requires_grad_(True)
    alone = {**plain, "t_enter": t_enter, "t_exit": t_exit}
    (radfoam.composite_segments(alone, density, rgb) * weights).sum().backward()
    ref64, ref32 = _restatements(seg, seg["exit_cells"], p, r, t_enter.grad, t_exit.grad)
    _assert_bars("autograd", r.grad.reshape(-1, 6).cpu().numpy(), ref64, ref32)

    p2, _, _, _, r2, _, seg2 = run(True, False)
    (radfoam.composite_segments(seg2, density, rgb) * weights).sum().backward()
    torch.cuda.synchronize()
    assert r2.grad is None
    nz = p2.grad[p2.grad != 0]
    assert torch.allclose(p.grad, p2.grad, rtol=1e-3, atol=1e-3 * float(nz.pow(2).mean().sqrt()))

    p3, _, _, _, r3, _, seg3 = run(False, True)
    assert seg3["t_exit"].grad_fn is not None
    (radfoam.composite_segments(seg3, density, rgb) * weights).sum().backward()
    torch.cuda.synchronize()
    assert p3.grad is None
    _assert_bars("autograd, rays alone", r3.grad.reshape(-1, 6).cpu().numpy(), ref64, ref32)

    *_, seg4 = run(False, False)
    assert seg4["t_enter"].grad_fn is None and seg4["t_exit"].grad_fn is None
    assert not seg4["t_enter"].requires_grad and not seg4["t_exit"].requires_grad
    with torch.no_grad():
        *_, seg5 = run(True, True)
    assert seg5["t_enter"].grad_fn is None and seg5["t_exit"].grad_fn is None


def test_leaves_the_trail_alone_with_rays_requiring_grad(foam_factory):
    fm, rays, starts, _ = S.image_case(foam_factory)
    inputs = _device_inputs(fm, rays, starts)
    g = torch.from_numpy(np.random.default_rng(4).normal(size=rays.shape[:-1] + (4,)).astype(np.float32)).to(DEV)
    pipe = _pipeline(2)
    pipe.record_trail = True
    fwd = pipe.trace_forward(*inputs)
    trail = pipe._trail
    assert trail is not None
    recorded = trail["trail"].clone()
    moving = inputs[4].clone().requires_grad_(True)
    seg = pipe.trace_differentiable_segments(*inputs[:4], moving, inputs[5], weight_threshold=0.5)
    assert seg["t_exit"].grad_fn is not None
    seg["t_exit"][torch.isfinite(seg["t_exit"])].sum().backward()
    assert moving.grad is not None and moving.grad.shape == moving.shape and bool((moving.grad != 0).any())
    assert pipe._trail is trail and torch.equal(trail["trail"], recorded)
    pipe.trace_backward(*inputs, fwd["rgba"], g)
    torch.cuda.synchronize()
    assert pipe.last_backward_replayed is True


def test_example_at_toy_size():
    from examples.fit_camera_pose import fit

    out = fit(num_points=2000, width=32, height=24, steps=8, log=lambda *_: None)
    losses = out["losses"]
    (angle0, shift0), (angle1, shift1) = out["error_before"], out["error_after"]
    print("mse", losses[0], "->", losses[-1], "rotation", angle0, "->", angle1, "translation", shift0, "->", shift1)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert angle1 < angle0 and shift1 < shift0
