"""radfoam.entry_weights on the GPU (rf_entry_weights.hip): the kernels against the float64 torch backend on
hand-built lists that put the carry across 64-entry steps, run heads at lane 0 and lane 63, empty rays at a wave's
boundary and a ray longer than a block's step where they can go wrong; an output left out of the loss; bitwise
reproducibility; the real walk against trace_forward's contribution and against composite_entries; and autograd from a
loss that is not linear in the weights down to points.grad and rays.grad.

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


def _hand_built(counts, seed):
    """The generator of tests/test_gpu_composite_entries.py without its values: per ray a random increasing sequence of
    times with zero-length (t_exit == t_enter) and inverted (t_exit < t_enter) crossings sprinkled in and +inf on some
    last entries; sigma in 0 .. 50 with exact zeros, scaled by 1.2 / n on a ray of n > 1 entries so that the sum of x
    over a ray stays near 2.5 and the last entries of a long ray still carry weight (what a carry gets wrong shows
    there)."""
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
    seg = {"offsets": torch.from_numpy(offsets).to(DEV), "t_enter": torch.from_numpy(t_enter).to(DEV),
           "t_exit": torch.from_numpy(t_exit).to(DEV)}
    return seg, torch.from_numpy(sigma).to(DEV)


def _leaves(seg, sigma, dtype):
    """Fresh leaves of `dtype` for all three differentiable inputs."""
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)
    s, t0, t1 = leaf(sigma), leaf(seg["t_enter"]), leaf(seg["t_exit"])
    return {**seg, "t_enter": t0, "t_exit": t1}, s, t0, t1


def _grads_in(total, seed):
    """(g_w, g_T) [S] float32, random normal."""
    rng = np.random.default_rng(seed)
    return tuple(torch.from_numpy(rng.normal(size=total).astype(np.float32)).to(DEV) for _ in range(2))


def _close(name, got, want):
    got, want = got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy()
    err = np.abs(got - want)
    bound = ATOL + RTOL * np.abs(want)
    print("%s: largest |kernel - float64 torch backend| %.3g, at %.3g of its bound; largest |reference| %.3g"
          % (name, err.max(initial=0.0), (err / bound).max(initial=0.0), np.abs(want).max(initial=0.0)))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=name)


def _reference(seg, sigma, g_w, g_t):
    """The float64 torch backend on the device: (weights, transmittance, {name: gradient}) for the incoming gradients
    (g_t None: the transmittance is left out of the loss)."""
    import radfoam

    seg64, s64, a64, b64 = _leaves(seg, sigma, torch.float64)
    weights, through = radfoam.entry_weights(seg64, s64, return_transmittance=True, backend="torch")
    assert weights.dtype == torch.float64 and through.dtype == torch.float64
    if weights.numel():
        loss = (weights * g_w.double()).sum() + (0 if g_t is None else (through * g_t.double()).sum())
        loss.backward()
    return weights.detach(), through.detach(), {"sigma": s64.grad, "t_enter": a64.grad, "t_exit": b64.grad}


def _check_grads(name, seg, grads, want, floor):
    """Every gradient at the bar, its reference's largest element between `floor` and 1e3, exact zeros behind infinite
    exits."""
    infinite = torch.isinf(seg["t_exit"])
    for key, got in grads.items():
        assert got is not None and got.dtype == torch.float32 and got.shape == want[key].shape
        # O(1) by construction, so that atol = 1e-7 is a float32 rounding of them and not a free pass
        if got.numel():
            assert floor < float(want[key].abs().max()) < 1e3, (name, key, float(want[key].abs().max()))
        _close(name + " grad " + key, got, want[key])
        assert bool((got[infinite] == 0).all()), (name, key)


def _check(name, seg, sigma, seed=1, floor=0.05):
    """Forward, both outputs, and all three gradients for random normal g_w and g_T against float64 autograd of the
    torch backend."""
    import radfoam

    total = sigma.numel()
    g_w, g_t = _grads_in(total, seed)
    seg32, s32, a32, b32 = _leaves(seg, sigma, torch.float32)
    weights, through = radfoam.entry_weights(seg32, s32, return_transmittance=True)
    assert "EntryWeights" in str(weights.grad_fn)
    for out in (weights, through):
        assert out.dtype == torch.float32 and out.shape == (total,) and out.is_cuda
    torch.autograd.backward([weights, through], [g_w, g_t])
    want_w, want_t, want = _reference(seg, sigma, g_w, g_t)
    torch.cuda.synchronize()
    _close(name + " weights", weights, want_w)
    _close(name + " transmittance", through, want_t)
    _check_grads(name, seg, {"sigma": s32.grad, "t_enter": a32.grad, "t_exit": b32.grad}, want, floor)
    infinite = torch.isinf(seg["t_exit"])
    assert bool((weights[infinite] == 0).all())
    counts = seg["offsets"][1:] - seg["offsets"][:-1]
    assert bool((through[seg["offsets"][:-1][counts > 0]] == 1).all())
    return weights.detach(), through.detach()


def test_hand_built_list():
    seg, sigma = _hand_built(COUNTS, seed=33)
    assert int(torch.isinf(seg["t_exit"]).sum()) >= 3 and bool((seg["t_exit"] == seg["t_enter"]).any())
    assert bool((seg["t_exit"] < seg["t_enter"]).any()) and bool((sigma == 0).any()) and float(sigma.max()) > 20
    weights, through = _check("hand-built", seg, sigma)
    last = seg["offsets"][-1] - 2                              # the long ray's last finite entry still carries weight
    assert float(weights.max()) > 0.3 and 1e-3 < float(through[last]) < 0.5


def test_only_the_weights_are_used():
    """return_transmittance=False, and True with the second output left out of the loss (its gradient reaches the
    kernel as a null pointer): at the bar, and the same bits as a run with g_T = 0 passed explicitly."""
    import radfoam

    seg, sigma = _hand_built(COUNTS, seed=34)
    g_w, _ = _grads_in(sigma.numel(), 2)
    want_w, _, want = _reference(seg, sigma, g_w, None)
    runs = []
    for mode in ("alone", "unused", "zeros"):
        seg32, s32, a32, b32 = _leaves(seg, sigma, torch.float32)
        if mode == "alone":
            weights = radfoam.entry_weights(seg32, s32)
            assert isinstance(weights, torch.Tensor)
            weights.backward(g_w)
        else:
            weights, through = radfoam.entry_weights(seg32, s32, return_transmittance=True)
            if mode == "unused":
                weights.backward(g_w)
            else:
                torch.autograd.backward([weights, through], [g_w, torch.zeros_like(g_w)])
        runs.append([weights.detach(), s32.grad, a32.grad, b32.grad])
    torch.cuda.synchronize()
    _close("weights alone", runs[0][0], want_w)
    _check_grads("weights alone", seg, dict(zip(("sigma", "t_enter", "t_exit"), runs[0][1:])), want, 0.05)
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert not bool(torch.isnan(a).any()) and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_one_ray_and_ray_counts_off_the_wave():
    """R = 1 with one entry; ray counts that are no multiple of the rays a wave owns, one below and one above a
    multiple, with short rays so that a wave's rays share a step; then R = 0, and S = 0 with R > 0."""
    import radfoam
    from radfoam_amd import _lib

    per_wave = int(_lib.load().rf_entry_weights_rays_per_wave())
    assert 1 <= per_wave <= 63
    # one entry gives one number per gradient: sigma = 15.9, dt = 0.072, g_w = 2.04; the smallest of them (to sigma) is
    # |g_w| exp(-x) dt = 0.047
    _check("one ray, one entry", *_hand_built([1], seed=8), seed=3, floor=0.01)
    rng = np.random.default_rng(3)
    for num_rays in (5 * per_wave - 1, 4 * per_wave + 1):
        assert num_rays % per_wave != 0
        counts = rng.integers(0, 40, size=num_rays)
        counts[-1] = 7
        _check("%d rays" % num_rays, *_hand_built(counts, seed=num_rays))
    for counts in ([], [0, 0, 0]):
        seg, sigma = _hand_built(counts, seed=4)
        assert sigma.numel() == 0 and seg["offsets"].numel() == len(counts) + 1
        seg32, s32, a32, b32 = _leaves(seg, sigma, torch.float32)
        weights, through = radfoam.entry_weights(seg32, s32, return_transmittance=True)
        for out in (weights, through):
            assert out.shape == (0,) and out.dtype == torch.float32 and out.is_cuda
        (weights.sum() + through.sum()).backward()
        assert s32.grad.shape == (0,) and a32.grad.shape == (0,) and b32.grad.shape == (0,)
        assert radfoam.entry_weights(seg, sigma).shape == (0,)


def test_needs_input_grad_subsets():
    import radfoam

    seg, sigma = _hand_built(COUNTS, seed=5)
    g_w, g_t = _grads_in(sigma.numel(), 6)
    full = _leaves(seg, sigma, torch.float32)
    torch.autograd.backward(list(radfoam.entry_weights(*full[:2], return_transmittance=True)), [g_w, g_t])
    want = dict(zip(("sigma", "t_enter", "t_exit"), (t.grad for t in full[1:])))
    for wanted in (("sigma",), ("t_enter", "t_exit"), ("t_enter",), ("t_exit",)):
        seg32, s, t0, t1 = _leaves(seg, sigma, torch.float32)
        leaves = {"sigma": s, "t_enter": t0, "t_exit": t1}
        for key, leaf in leaves.items():
            leaf.requires_grad_(key in wanted)
        torch.autograd.backward(list(radfoam.entry_weights(seg32, s, return_transmittance=True)), [g_w, g_t])
        torch.cuda.synchronize()
        for key, leaf in leaves.items():
            if key in wanted:                 # no atomics: the same bits whichever other gradients are computed
                assert torch.equal(leaf.grad.view(torch.int32), want[key].view(torch.int32)), (wanted, key)
            else:
                assert leaf.grad is None, (wanted, key)


def test_bitwise_reproducible():
    import radfoam

    seg, sigma = _hand_built(COUNTS, seed=7)
    g_w, g_t = _grads_in(sigma.numel(), 8)
    runs = []
    for _ in range(2):
        leaves = _leaves(seg, sigma, torch.float32)
        weights, through = radfoam.entry_weights(*leaves[:2], return_transmittance=True)
        torch.autograd.backward([weights, through], [g_w, g_t])
        runs.append([weights.detach(), through.detach()] + [t.grad for t in leaves[1:]])
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert not bool(torch.isnan(a).any()) and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _device_inputs(fm, rays, starts):
    p, a, adj, off = H.to_torch_foam(fm, DEV)
    r = torch.from_numpy(np.ascontiguousarray(rays)).to(DEV)
    s = torch.from_numpy(np.ascontiguousarray(starts, dtype=np.uint32)).to(DEV)
    return p, a, adj, off, r, s


def _real_walk(foam_factory):
    """The degree-0 foam of 3000 points under the 64x48 camera, as tests/test_gpu_cell_entries.py builds it."""
    import radfoam

    fm, rays, starts, _ = S.image_case(foam_factory, sh_degree=0)
    p, a, adj, off, r, s = _device_inputs(fm, rays, starts)
    pipe = radfoam.create_pipeline(0)
    seg = pipe.trace_segments(p, a, adj, off, r, s)
    index = radfoam.cell_entries(seg, p.size(0))
    lengths = index.cell_offsets[1:] - index.cell_offsets[:-1]
    assert int(lengths.max()) == r.numel() // 6 == 3072 and int(lengths[int(starts.reshape(-1)[0])]) == 3072
    return pipe, (p, a, adj, off, r, s), seg, index


def test_real_walk_contribution_against_trace_forward(foam_factory):
    """The kernel's weights of the pipeline's own walk, summed per cell by reduce_entries, against the pipeline's
    trace_forward(return_contribution=True): DESIGN section 2's bar for scatter outputs, 1e-3 per element and 1e-5
    relative L2, over every cell."""
    import radfoam

    pipe, inputs, seg, index = _real_walk(foam_factory)
    ref = pipe.trace_forward(*inputs, return_contribution=True)["contribution"].reshape(-1).double()
    sigma = inputs[1][:, -1].float()[index.cells]
    weights = radfoam.entry_weights(seg, sigma)
    assert weights.dtype == torch.float32 and weights.is_cuda
    got = radfoam.reduce_entries(index, weights)
    torch.cuda.synchronize()
    err = (got.double() - ref).abs()
    rel = float((err ** 2).sum().sqrt() / (ref ** 2).sum().sqrt())
    print("%d entries; %d cells of non-zero contribution, the largest %.3g; largest difference %.3g, at %.3g of its "
          "bound; relative L2 %.3g, at %.3g of its bound"
          % (index.cells.numel(), int((ref != 0).sum()), float(ref.max()), float(err.max()), float(err.max()) / 1e-3,
             rel, rel / 1e-5))
    assert got.shape == ref.shape and int((ref != 0).sum()) > 500 and float(ref.max()) > 1
    assert float(err.max()) <= 1e-3 and rel <= 1e-5


def test_real_walk_against_composite_entries(foam_factory):
    """sum_e w_e values[e][c] per ray, with the kernel's float32 w_e and the sum in float64, against composite_entries'
    kernel on the same inputs.  Both form w_e in double by the same operations.  Here every w_e is rounded to float32
    (relative error at most u = 2^-24) before an exact-to-1e-16 sum, there the sum is rounded once, so
        |difference| <= u sum_e |w_e values[e][c]| + u |out| <= u (1 + |out|),
    as |values| <= 1 and a ray's weights sum to at most 1.  That lies within the project's bar plus one float32 rounding
    of the per-ray sum, 1e-7 + (2e-7 + 2^-24) |out|, which is what is asserted."""
    import radfoam

    _, inputs, seg, index = _real_walk(foam_factory)
    total, num_rays, channels = index.cells.numel(), 3072, 3
    sigma = inputs[1][:, -1].float()[index.cells].contiguous()
    values = torch.from_numpy(np.random.default_rng(9).uniform(-1.0, 1.0, size=(total, channels)).astype(np.float32))
    values = values.to(DEV)
    weights = radfoam.entry_weights(seg, sigma)
    want = radfoam.composite_entries(seg, sigma, values)[:, :channels].double()
    counts = seg["offsets"][1:] - seg["offsets"][:-1]
    ray = torch.repeat_interleave(torch.arange(num_rays, device=DEV), counts, output_size=total)
    got = torch.zeros((num_rays, channels), dtype=torch.float64, device=DEV).index_add(
        0, ray, weights.double().unsqueeze(-1) * values.double())
    torch.cuda.synchronize()
    err = (got - want).abs()
    bound = ATOL + (RTOL + 2.0 ** -24) * want.abs()
    print("largest |sum of w values - composite_entries| %.3g, at %.3g of its bound; largest |composite_entries| %.3g"
          % (float(err.max()), float((err / bound).max()), float(want.abs().max())))
    assert float(want.abs().max()) > 0.3 and bool((err <= bound).all())


def test_autograd_end_to_end(foam_factory):
    """points and rays requiring grad, trace_differentiable_segments, entry_weights with both outputs, a loss that is
    not linear in the weights (the ray entropy -sum w log(w + 1e-8), plus a random linear term in T), .backward(): the
    float32 kernels against the float64 torch backend.  Both chains end in the same atomic kernels, so the criterion is
    test_autograd_end_to_end's of tests/test_gpu_segments_grad.py: per element 1e-3 |ref| + 1e-3 rms."""
    import radfoam

    fm, rays, starts, _ = S.image_case(foam_factory)
    density = torch.from_numpy((fm["attributes"][:, -1] + 0.2).astype(np.float32)).to(DEV)
    pipe = radfoam.create_pipeline(2)
    linear = {}

    def run(dtype, backend):
        p, a, adj, off, r, s = _device_inputs(fm, rays, starts)
        p.requires_grad_(True)
        r.requires_grad_(True)
        seg = pipe.trace_differentiable_segments(p, a, adj, off, r, s, weight_threshold=0.5)
        assert seg["t_exit"].grad_fn is not None
        sigma = density[seg["cells"].to(torch.int64)].to(dtype)
        if not linear:
            linear["c"] = torch.from_numpy(np.random.default_rng(13).normal(size=sigma.numel())).to(DEV)
        weights, through = radfoam.entry_weights(seg, sigma, return_transmittance=True, backend=backend)
        assert weights.dtype == dtype and ("EntryWeights" in str(weights.grad_fn)) == (backend is None)
        loss = -(weights * torch.log(weights + 1e-8)).sum() + (through * linear["c"].to(dtype)).sum()
        loss.backward()
        torch.cuda.synchronize()
        return p.grad.cpu().numpy(), r.grad.reshape(-1, 6).cpu().numpy()

    got = run(torch.float32, None)
    want = run(torch.float64, "torch")
    for name, g, w in zip(("points.grad", "rays.grad"), got, want):
        assert g.dtype == np.float32 and g.shape == w.shape and np.abs(w).max() > 0
        finite = np.isfinite(w)
        assert np.isfinite(g[finite]).all() and finite.mean() > 0.99
        g, w = g[finite], w[finite]
        ok, rel, worst = H.grad_close(g, w)
        print("%s: relative L2 to the chain through the float64 torch backend %.3g, worst element at %.3g of its bound"
              % (name, rel, worst))
        assert ok, (name, worst)


def test_example_at_toy_size():
    from examples.weight_entropy import run

    out = run(num_points=2000, width=32, height=24, steps=3, log=lambda *_: None)
    contribution = out["contribution"]
    print("mse %.4g without, %.4g with the term; mean ray entropy %.4g without, %.4g with; contribution: sum %.4g, "
          "largest %.4g" % (out["mse_without"], out["mse_with"], out["entropy_without"], out["entropy_with"],
                            float(contribution.sum()), float(contribution.max())))
    for key in ("mse_without", "mse_with", "entropy_without", "entropy_with"):
        assert np.isfinite(out[key]), key
    assert contribution.shape == (2000,) and contribution.dtype == torch.float32
    assert bool(torch.isfinite(contribution).all()) and bool((contribution >= 0).all())
    assert bool(torch.isfinite(out["error"]).all())
    # every ray's weights sum to its opacity: at most one per ray
    assert 0 < float(contribution.sum()) <= 32 * 24 * (1 + 1e-5)
    assert out["entropy_with"] <= out["entropy_without"]
