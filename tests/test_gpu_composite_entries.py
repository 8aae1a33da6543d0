"""radfoam.composite_entries on the GPU (rf_composite.hip): the kernels against the float64 torch backend
on hand-built lists that put the carry across 64-entry steps, run heads at lane 0 and lane 63, empty rays at a wave's
boundary and a ray longer than a block where they can go wrong; bitwise reproducibility; the real walk against
composite_segments and trace_forward; and autograd from a composited loss down to points.grad and rays.grad.

The bar is the project's for a result computed in double and rounded once to float32: rtol = 2e-7, atol = 1e-7 (half
a float32 ulp is 6e-8 relative)."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import segments_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RTOL, ATOL = 2e-7, 1e-7
COUNTS = [0, 1, 63, 64, 65, 0, 0, 130, 1, 300, 0, 2, 1024]


def _hand_built(counts, channels, seed):
    """A list with the given entries per ray: per ray a random increasing sequence of times with zero-length
    (t_exit == t_enter) and inverted (t_exit < t_enter) crossings sprinkled in and +inf on some last entries; sigma in
    0 .. 50 with exact zeros, scaled by 1.2 / n on a ray of n > 1 entries so that the sum of x over a ray stays near 2.5
    and the last entries of a long ray still carry weight (what a carry gets wrong shows there); values in -1 .. 1."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, dtype=np.int64)
    total = int(counts.sum())
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    t_enter, t_exit, sigma = np.zeros(total, np.float32), np.zeros(total, np.float32), np.zeros(total, np.float32)
    for r, n in enumerate(counts):
        if n == 0:
            continue
        lo = offsets[r]
        steps = rng.uniform(0.01, 0.2, size=n)
        edges = np.concatenate([[0.0], np.cumsum(steps)]).astype(np.float32)
        t_enter[lo:lo + n], t_exit[lo:lo + n] = edges[:-1], edges[1:]
        kind = rng.uniform(size=n)
        flat, inverted = kind < 0.08, (kind >= 0.08) & (kind < 0.16)
        t_exit[lo:lo + n][flat] = t_enter[lo:lo + n][flat]
        t_exit[lo:lo + n][inverted] = t_enter[lo:lo + n][inverted] - np.float32(0.05)
        if r % 2 == 1 or n == 1024:
            t_exit[lo + n - 1] = np.inf
        s = rng.uniform(0.0, 50.0, size=n) * (rng.uniform(size=n) > 0.15)
        sigma[lo:lo + n] = s * min(1.0, 1.2 / n)
    values = rng.uniform(-1.0, 1.0, size=(total, channels)).astype(np.float32)
    seg = {"offsets": torch.from_numpy(offsets).to(DEV), "t_enter": torch.from_numpy(t_enter).to(DEV),
           "t_exit": torch.from_numpy(t_exit).to(DEV)}
    return seg, torch.from_numpy(sigma).to(DEV), torch.from_numpy(values).to(DEV)


def _leaves(seg, sigma, values, dtype):
    """Fresh leaves of `dtype` for all four differentiable inputs."""
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)
    s, v, t0, t1 = leaf(sigma), leaf(values), leaf(seg["t_enter"]), leaf(seg["t_exit"])
    return {**seg, "t_enter": t0, "t_exit": t1}, s, v, t0, t1


def _close(name, got, want):
    got, want = got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy()
    err = np.abs(got - want)
    bound = ATOL + RTOL * np.abs(want)
    print("%s: largest |kernel - float64 torch backend| %.3g, at %.3g of its bound; largest |reference| %.3g"
          % (name, err.max(initial=0.0), (err / bound).max(initial=0.0), np.abs(want).max(initial=0.0)))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=name)


def _check(name, seg, sigma, values, seed=1, floor=0.05):
    """Forward and all four gradients for a random G against float64 autograd of the torch backend.  The largest
    element of every gradient must lie between `floor` and 1e3."""
    import radfoam

    num_rays, channels = seg["offsets"].numel() - 1, values.size(1)
    g = torch.from_numpy(np.random.default_rng(seed).normal(size=(num_rays, channels + 1))).to(DEV)
    seg32, s32, v32, a32, b32 = _leaves(seg, sigma, values, torch.float32)
    out = radfoam.composite_entries(seg32, s32, v32)
    assert out.dtype == torch.float32 and out.shape == (num_rays, channels + 1) and out.is_cuda
    out.backward(g.float())
    seg64, s64, v64, a64, b64 = _leaves(seg, sigma, values, torch.float64)
    ref = radfoam.composite_entries(seg64, s64, v64, backend="torch")
    assert ref.dtype == torch.float64
    ref.backward(g.float().double())
    torch.cuda.synchronize()
    _close(name + " forward", out, ref)
    grads = {"sigma": (s32.grad, s64.grad), "values": (v32.grad, v64.grad), "t_enter": (a32.grad, a64.grad),
             "t_exit": (b32.grad, b64.grad)}
    for key, (got, want) in grads.items():
        assert got is not None and got.dtype == torch.float32 and got.shape == want.shape
        # O(1) by construction, so that atol = 1e-7 is a float32 rounding of them and not a free pass
        if want.numel():
            assert floor < float(want.abs().max()) < 1e3, (name, key, float(want.abs().max()))
        _close(name + " grad " + key, got, want)
    infinite = torch.isinf(seg["t_exit"])
    if bool(infinite.any()):
        for key, (got, _) in grads.items():
            assert bool((got[infinite] == 0).all()), (name, key)
    counts = seg["offsets"][1:] - seg["offsets"][:-1]
    assert bool((out[counts == 0] == 0).all())
    return out


@pytest.mark.parametrize("channels", [1, 3, 4, 5, 16])
def test_hand_built_list(channels):
    seg, sigma, values = _hand_built(COUNTS, channels, seed=30 + channels)
    assert bool(torch.isinf(seg["t_exit"]).any()) and bool((seg["t_exit"] == seg["t_enter"]).any())
    assert bool((seg["t_exit"] < seg["t_enter"]).any()) and bool((sigma == 0).any()) and float(sigma.max()) > 20
    out = _check("hand-built, C = %d" % channels, seg, sigma, values)
    assert float(out[:, -1].max()) > 0.8 and int((out[:, -1] > 0.2).sum()) >= 6


def test_one_ray_and_ray_counts_off_the_wave():
    """R = 1 with one entry; then ray counts that are no multiple of the rays a wave owns, one below and one above a
    multiple, with short rays so that a wave's rays share a step."""
    from radfoam_amd import _lib

    per_wave = int(_lib.load().rf_composite_rays_per_wave())
    assert 1 <= per_wave <= 63
    # one entry gives one number per gradient: sigma = 15.9, dt = 0.17, the smallest of them (to sigma) is 0.029
    _check("one ray, one entry", *_hand_built([1], 3, seed=8), floor=0.01)
    rng = np.random.default_rng(3)
    for num_rays in (5 * per_wave - 1, 4 * per_wave + 1):
        assert num_rays % per_wave != 0
        counts = rng.integers(0, 40, size=num_rays)
        counts[-1] = 7
        _check("%d rays" % num_rays, *_hand_built(counts, 3, seed=num_rays))


def test_needs_input_grad_subsets():
    import radfoam

    seg, sigma, values = _hand_built(COUNTS, 3, seed=5)
    g = torch.from_numpy(np.random.default_rng(6).normal(size=(len(COUNTS), 4)).astype(np.float32)).to(DEV)
    full = _leaves(seg, sigma, values, torch.float32)
    radfoam.composite_entries(*full[:3]).backward(g)
    want = dict(zip(("sigma", "values", "t_enter", "t_exit"), (t.grad for t in full[1:])))
    for wanted in (("values",), ("sigma",), ("t_enter", "t_exit"), ("t_enter",), ("t_exit",)):
        seg32, s, v, t0, t1 = _leaves(seg, sigma, values, torch.float32)
        leaves = {"sigma": s, "values": v, "t_enter": t0, "t_exit": t1}
        for key, leaf in leaves.items():
            leaf.requires_grad_(key in wanted)
        radfoam.composite_entries(seg32, s, v).backward(g)
        torch.cuda.synchronize()
        for key, leaf in leaves.items():
            if key in wanted:                 # no atomics: the same bits whichever other gradients are computed
                assert torch.equal(leaf.grad.view(torch.int32), want[key].view(torch.int32)), (wanted, key)
            else:
                assert leaf.grad is None, (wanted, key)


def test_bitwise_reproducible():
    import radfoam

    seg, sigma, values = _hand_built(COUNTS, 5, seed=7)
    g = torch.from_numpy(np.random.default_rng(8).normal(size=(len(COUNTS), 6)).astype(np.float32)).to(DEV)
    runs = []
    for _ in range(2):
        leaves = _leaves(seg, sigma, values, torch.float32)
        out = radfoam.composite_entries(*leaves[:3])
        out.backward(g)
        runs.append([out.detach()] + [t.grad for t in leaves[1:]])
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert not bool(torch.isnan(a).any()) and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _device_inputs(fm, rays, starts):
    p, a, adj, off = H.to_torch_foam(fm, DEV)
    r = torch.from_numpy(np.ascontiguousarray(rays)).to(DEV)
    s = torch.from_numpy(np.ascontiguousarray(starts, dtype=np.uint32)).to(DEV)
    return p, a, adj, off, r, s


def test_real_walk_against_composite_segments(foam_factory):
    import radfoam

    fm, rays, starts, ref = S.image_case(foam_factory)
    seg = radfoam.create_pipeline(2).trace_segments(*_device_inputs(fm, rays, starts))
    assert seg["cells"].numel() == 78222 and int((seg["offsets"][1:] - seg["offsets"][:-1]).max()) == 35
    rng = np.random.default_rng(9)
    density = torch.from_numpy(fm["attributes"][:, -1].astype(np.float32)).to(DEV)
    rgb = torch.from_numpy(rng.uniform(0.0, 1.0, size=(density.numel(), 3)).astype(np.float32)).to(DEV)
    cells = seg["cells"].to(torch.int64)
    got = radfoam.composite_entries(seg, density[cells], rgb[cells])
    want = radfoam.composite_segments(seg, density.double(), rgb.double())
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and float(want[:, 3].min()) < 0.5 < float(want[:, 3].max())
    _close("image case", got, want)


def test_reproduces_trace_forward(foam_factory):
    """The degree-0 foam of test_composite_segments_reproduces_trace_forward, with trace_forward's colour model per
    entry, against trace_forward's fp32 rgba: within 1e-4 absolute, that test's bar."""
    import radfoam

    fm = foam_factory(3000, 0, 21)
    _, rays, start = H.camera_setup(fm, 64, 48)
    inputs = _device_inputs(fm, rays, np.full(rays.shape[:-1], start, dtype=np.uint32))
    density = torch.from_numpy(fm["attributes"][:, 3].astype(np.float32)).to(DEV)
    rgb = torch.from_numpy(S.flat_colour(fm["attributes"]).astype(np.float32)).to(DEV)
    pipe = radfoam.create_pipeline(0)
    for kw in ({}, {"weight_threshold": 0.5}):
        seg = pipe.trace_segments(*inputs, **kw)
        cells = seg["cells"].to(torch.int64)
        got = radfoam.composite_entries(seg, density[cells], rgb[cells]).double()
        want = pipe.trace_forward(*inputs, **kw)["rgba"].reshape(-1, 4).double()
        assert got.shape == want.shape
        worst = float((got - want).abs().max())
        print(kw, "largest |composite_entries - trace_forward|:", worst)
        assert float(want[:, 3].max()) > 0.5 and worst <= 1e-4


def test_autograd_end_to_end(foam_factory):
    """points and rays requiring grad, trace_differentiable_segments, composite_entries, .square().sum().backward():
    against the same chain through composite_segments.  Both chains end in the same atomic kernels, so the criterion is
    test_autograd_end_to_end's of tests/test_gpu_segments_grad.py: per element 1e-3 |ref| + 1e-3 rms."""
    import radfoam

    fm, rays, starts, _ = S.image_case(foam_factory)
    rng = np.random.default_rng(13)
    density = torch.from_numpy((fm["attributes"][:, -1] + 0.2).astype(np.float32)).to(DEV)
    rgb = torch.from_numpy(rng.uniform(0.0, 1.0, size=(density.numel(), 3)).astype(np.float32)).to(DEV)
    pipe = radfoam.create_pipeline(2)

    def run(composite):
        p, a, adj, off, r, s = _device_inputs(fm, rays, starts)
        p.requires_grad_(True)
        r.requires_grad_(True)
        seg = pipe.trace_differentiable_segments(p, a, adj, off, r, s, weight_threshold=0.5)
        assert seg["t_exit"].grad_fn is not None
        composite(seg).square().sum().backward()
        torch.cuda.synchronize()
        return p.grad.cpu().numpy(), r.grad.reshape(-1, 6).cpu().numpy()

    def entries(seg):
        cells = seg["cells"].to(torch.int64)
        return radfoam.composite_entries(seg, density[cells], rgb[cells])

    got = run(entries)
    want = run(lambda seg: radfoam.composite_segments(seg, density, rgb))
    for name, g, w in zip(("points.grad", "rays.grad"), got, want):
        assert g.dtype == np.float32 and g.shape == w.shape and np.abs(w).max() > 0
        finite = np.isfinite(w)
        assert np.isfinite(g[finite]).all() and finite.mean() > 0.99
        g, w = g[finite], w[finite]
        ok, rel, worst = H.grad_close(g, w)
        print("%s: relative L2 to the chain through composite_segments %.3g, worst element at %.3g of its bound"
              % (name, rel, worst))
        assert ok, (name, worst)


def test_example_at_toy_size():
    from examples.view_dependent_shading import fit

    first, last = fit(num_points=2000, width=32, height=24, steps=10, log=lambda *_: None)
    print("mse", first, "->", last)
    assert np.isfinite(first) and np.isfinite(last) and last < first
