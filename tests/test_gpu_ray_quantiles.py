"""radfoam.ray_quantiles on the GPU (rf_quantiles.hip): the kernels against the float64 torch backend on
hand-built lists whose levels are placed so that quantiles are crossed in a ray's first and last entry, in lanes 0 and 63
of a 64-entry step, behind one and several carries and deep inside a ray longer than a block; small cases; bitwise
reproducibility; the limit on the number of quantiles; the real walk against trace_forward(depth_quantiles=...); and
autograd from a quantile-gap loss down to points.grad and rays.grad.

The bar is the project's for a result computed in double and rounded once to float32: rtol = 2e-7, atol = 1e-7 (half a
float32 ulp is 6e-8 relative; both sides read the same float32 inputs), and the entries must be equal.  Equality is a
fair demand because every test first asserts, from the torch backend's own numbers, that no level lies within 1e-9
(relative) of an inclusive sum of its ray: the two backends sum x in different orders and differ by about 1e-16 there.
(A level of exactly 0 against an inclusive sum of exactly 0, in front of a ray's first weight, is no such case: a sum of
zeros is 0 in any order.)"""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import segments_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RTOL, ATOL = 2e-7, 1e-7
COUNTS = [0, 1, 63, 64, 65, 0, 0, 130, 1, 300, 0, 2, 1024]
KEYS = ("sigma", "t_enter", "t_exit")


def _hand_built(counts, seed, dev=DEV):
    """The generator of tests/test_gpu_ray_distortion.py, restated: per ray a random increasing sequence of times with
    zero-length (t_exit == t_enter) and inverted (t_exit < t_enter) crossings sprinkled in and +inf on some last
    entries; sigma is 0 for one entry in seven and else drawn from 5 .. 50, scaled by 1.2 / n on a ray of n > 1 entries
    so that the sum of x over a ray stays near 3 and dt / sigma at a crossing stays moderate.  The first and the last
    finite entry of every ray, and every entry in lane 0 or 63 of a 64-entry step, carry weight (a positive length and
    density), so that levels can be placed in them."""
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
        k = np.arange(lo, lo + n)
        kind = rng.uniform(size=n)
        keep = (k == lo) | (k >= lo + n - 2) | (k % 64 == 0) | (k % 64 == 63)
        flat, inverted = (kind < 0.08) & ~keep, (kind >= 0.08) & (kind < 0.16) & ~keep
        t_enter[lo:lo + n], t_exit[lo:lo + n] = edges[:-1], edges[1:]
        t_exit[lo:lo + n][flat] = t_enter[lo:lo + n][flat]
        t_exit[lo:lo + n][inverted] = t_enter[lo:lo + n][inverted] - np.float32(0.05)
        if r % 2 == 1 or n == 1024:
            t_exit[lo + n - 1] = np.inf
        s = rng.uniform(5.0, 50.0, size=n) * ((rng.uniform(size=n) > 0.15) | keep)
        sigma[lo:lo + n] = s * min(1.0, 1.2 / n)
    seg = {"offsets": torch.from_numpy(offsets).to(dev), "t_enter": torch.from_numpy(t_enter).to(dev),
           "t_exit": torch.from_numpy(t_exit).to(dev)}
    return seg, torch.from_numpy(sigma).to(dev)


def _sums(seg, sigma):
    """float64 on the CPU, from the widened float32 inputs: (offsets, x [S], the inclusive sum I [S] of every entry
    within its ray as the torch backend forms it, the ray of every entry)."""
    off = seg["offsets"].cpu()
    t_enter, t_exit, sig = seg["t_enter"].detach().cpu().double(), seg["t_exit"].detach().cpu().double(), sigma.detach().cpu().double()
    dt = torch.where(torch.isinf(t_exit), torch.zeros_like(t_exit), (t_exit - t_enter).clamp_min(0.0))
    x = sig * dt
    run0 = torch.cat([x.new_zeros(1), torch.cumsum(x, 0)])
    ray = torch.repeat_interleave(torch.arange(off.numel() - 1), off[1:] - off[:-1])
    return off.numpy(), x.numpy(), (run0[1:] - run0[off[:-1]][ray]).numpy(), ray.numpy()


def _placed_quantiles(seg, sigma, num_q, seed, dev=DEV):
    """[R, Q] float32 quantiles q = exp(-L) with L placed from the ray's own float64 sums.  Column 0 holds, ray by ray,
    the placements the kernel can get wrong; the other columns cycle through u X_total with u = 0 (q = 1), 0.999, 1.5
    (never reached) and random values.  A placed level lies in the middle of its entry: L = I_k - x_k / 2."""
    rng = np.random.default_rng(seed)
    off, x, upto, _ = _sums(seg, sigma)
    num_rays = len(off) - 1
    level = np.zeros((num_rays, num_q))

    def inside(k):
        assert x[k] > 0, k
        return upto[k] - 0.5 * x[k]

    for r in range(num_rays):
        lo, hi = off[r], off[r + 1]
        n = hi - lo
        total = upto[hi - 1] if n else 1.0
        steps_in = [k for k in range(lo, hi) if k % 64 == 0 and k > lo]          # lane 0 of the ray's later steps
        column0 = {63: lambda: inside(hi - 1),               # ends in lane 63 of the first step: its last entry
                   64: lambda: 0.0,                          # q = 1: its first entry, lane 0
                   65: lambda: inside(hi - 1),               # its last entry, lane 0 of the step behind one carry
                   130: lambda: inside(steps_in[-1]),        # lane 0 behind two carries
                   300: lambda: inside(steps_in[2] - 1),     # lane 63 of a middle step
                   1024: lambda: inside(steps_in[-2]),       # deep in the ray that is longer than a block
                   2: lambda: 0.999 * total, 1: lambda: 0.5 * total}
        for q in range(num_q):
            if n == 0:
                level[r, q] = rng.uniform(0.1, 2.0)
            elif q == 0 and n in column0:
                level[r, q] = column0[n]()
            else:
                u = (0.0, 0.999, 1.5)[(q + r) % 6] if (q + r) % 6 < 3 else rng.uniform(0.02, 0.98)
                level[r, q] = u * total
    return torch.from_numpy(np.exp(-level).astype(np.float32)).to(dev)


def _random_quantiles(seg, sigma, num_q, seed, dev=DEV):
    """[R, Q] float32: exp(-u X_total) with u among 0, 0.999, 1.5 and random values."""
    rng = np.random.default_rng(seed)
    off, _, upto, _ = _sums(seg, sigma)
    total = np.array([upto[off[r + 1] - 1] if off[r + 1] > off[r] else 1.0 for r in range(len(off) - 1)])
    u = rng.uniform(0.02, 0.98, size=(len(total), num_q))
    special = rng.uniform(size=u.shape)
    u = np.where(special < 0.1, 0.0, np.where(special < 0.2, 0.999, np.where(special < 0.3, 1.5, u)))
    return torch.from_numpy(np.exp(-u * total[:, None]).astype(np.float32)).to(dev)


def _assert_levels_are_clear(seg, sigma, quantiles):
    """No level within 1e-9 (relative) of an inclusive sum of its ray, in the torch backend's own float64 numbers."""
    from radfoam_amd.segments import _quantile_levels

    off, _, upto, ray = _sums(seg, sigma)
    levels = _quantile_levels(quantiles.detach().cpu(), len(off) - 1, quantiles.size(-1)).numpy()
    for q in range(levels.shape[1]):
        level = levels[ray, q]
        finite = np.isfinite(level)
        near = np.abs(upto - level) <= 1e-9 * np.maximum(np.abs(upto), np.abs(level))
        near &= finite & ~((upto == 0) & (level == 0))
        assert not near.any(), (q, np.nonzero(near)[0][:5])


def _leaves(seg, sigma, dtype):
    """Fresh leaves of `dtype` for every differentiable input: (seg, dict of the leaves by name)."""
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)
    leaves = {"sigma": leaf(sigma), "t_enter": leaf(seg["t_enter"]), "t_exit": leaf(seg["t_exit"])}
    return {**seg, "t_enter": leaves["t_enter"], "t_exit": leaves["t_exit"]}, leaves


def _close(name, got, want):
    got, want = got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy()
    err = np.abs(got - want)
    bound = ATOL + RTOL * np.abs(want)
    print("%s: largest |kernel - float64 torch backend| %.3g, at %.3g of its bound; largest |reference| %.3g"
          % (name, err.max(initial=0.0), (err / bound).max(initial=0.0), np.abs(want).max(initial=0.0)))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=name)


def _check(name, seg, sigma, quantiles, seed=1, g=None, magnitudes=True):
    """Forward and every gradient for G (random where not given) against float64 autograd of the torch backend.  The
    largest element of every gradient must lie between 0.05 and 1e3."""
    import radfoam

    _assert_levels_are_clear(seg, sigma, quantiles)
    num_rays, num_q = seg["offsets"].numel() - 1, quantiles.size(-1)
    g = np.random.default_rng(seed).normal(size=(num_rays, num_q)) if g is None else np.asarray(g, dtype=np.float64)
    g = torch.from_numpy(g).to(DEV)
    seg32, l32 = _leaves(seg, sigma, torch.float32)
    depth, entries = radfoam.ray_quantiles(seg32, l32["sigma"], quantiles)
    assert depth.dtype == torch.float32 and depth.shape == (num_rays, num_q) and depth.is_cuda
    assert entries.dtype == torch.int64 and entries.shape == (num_rays, num_q) and not entries.requires_grad
    assert depth.grad_fn is not None
    depth.backward(g.float())
    seg64, l64 = _leaves(seg, sigma, torch.float64)
    ref, ref_entries = radfoam.ray_quantiles(seg64, l64["sigma"], quantiles.double(), backend="torch")
    assert ref.dtype == torch.float64
    ref.backward(g.float().double())
    torch.cuda.synchronize()
    assert torch.equal(entries, ref_entries), name
    assert bool(((depth == -1) == (entries == -1)).all())
    _close(name + " forward", depth, ref)
    for key in KEYS:
        got, want = l32[key].grad, l64[key].grad
        assert got is not None and got.dtype == torch.float32 and got.shape == want.shape
        # O(1) by construction, so that atol = 1e-7 is a float32 rounding of them and not a free pass
        if magnitudes:
            assert 0.05 < float(want.abs().max()) < 1e3, (name, key, float(want.abs().max()))
        _close(name + " grad " + key, got, want)
    infinite = torch.isinf(seg["t_exit"])
    if bool(infinite.any()):
        for key in KEYS:
            assert bool((l32[key].grad[infinite] == 0).all()), (name, key)
    assert all(bool(torch.isfinite(t.grad).all()) for t in l32.values()) and bool(torch.isfinite(depth).all())
    counts = seg["offsets"][1:] - seg["offsets"][:-1]
    assert bool((entries[counts == 0] == -1).all())
    return depth, entries


def _max_quantiles():
    from radfoam_amd import _lib

    return int(_lib.load().rf_quantiles_max())


@pytest.mark.parametrize("num_q", [1, 2, 3, "most"])
def test_hand_built_list(num_q):
    num_q = _max_quantiles() if num_q == "most" else num_q
    seg, sigma = _hand_built(COUNTS, seed=40)
    assert bool(torch.isinf(seg["t_exit"]).any()) and bool((seg["t_exit"] == seg["t_enter"]).any())
    assert bool((seg["t_exit"] < seg["t_enter"]).any()) and bool((sigma == 0).any()) and float(sigma.max()) > 20
    quantiles = _placed_quantiles(seg, sigma, num_q, seed=41)
    _, entries = _check("hand-built, Q = %d" % num_q, seg, sigma, quantiles)
    entries, off = entries.cpu().numpy(), seg["offsets"].cpu().numpy()
    first, last = off[:-1, None], off[1:, None] - 1
    found = entries >= 0
    steps_behind = entries // 64 - first // 64             # the carries in front of a crossing
    assert (found & (entries == first)).any(), "no crossing in a ray's first entry"
    assert (found & (entries == last)).any(), "no crossing in a ray's last entry"
    assert (found & (entries % 64 == 63)).any() and (found & (entries % 64 == 0)).any(), "lanes 63 and 0"
    assert (found & (steps_behind == 1)).any() and (found & (steps_behind >= 2)).any(), "behind one and more carries"
    assert found[12].any() and steps_behind[12][found[12]].max() >= 8, "the 1024-entry ray's later steps"
    assert (~found).sum() >= 5 and found.sum() >= 6


def test_one_ray_and_ray_counts_off_the_wave():
    """R = 1 with one entry; then ray counts that are no multiple of the rays a wave owns, one below and one above a
    multiple, with short rays so that a wave's rays share a step."""
    from radfoam_amd import _lib

    per_wave = int(_lib.load().rf_quantiles_rays_per_wave())
    assert 1 <= per_wave <= 63
    # one entry: x = 2, the median lies at L = 0.69: depth = 0.5 + 0.69 / 1; the gradients are G (-0.69, 1, nothing):
    # t_exit of a crossing entry gets an exact 0, so the magnitudes are not asserted here
    seg = {"offsets": torch.tensor([0, 1], device=DEV), "t_enter": torch.tensor([0.5], device=DEV),
           "t_exit": torch.tensor([2.5], device=DEV)}
    sigma = torch.ones(1, device=DEV)
    depth, entries = _check("one ray, one entry", seg, sigma, torch.tensor([[0.5, 0.01]], device=DEV), g=[[2.0, 1.0]],
                            magnitudes=False)
    assert entries.tolist() == [[0, -1]] and abs(float(depth.detach()[0, 0]) - (0.5 + np.log(2.0))) < 1e-6
    rng = np.random.default_rng(3)
    for num_rays in (5 * per_wave - 1, 4 * per_wave + 1):
        assert num_rays % per_wave != 0
        counts = rng.integers(0, 40, size=num_rays)
        counts[-1] = 7
        seg, sigma = _hand_built(counts, seed=num_rays)
        _check("%d rays" % num_rays, seg, sigma, _random_quantiles(seg, sigma, 2, seed=num_rays + 1))


def test_needs_input_grad_subsets_and_bitwise_reproducible():
    import radfoam

    seg, sigma = _hand_built(COUNTS, seed=5)
    quantiles = _random_quantiles(seg, sigma, 3, seed=6)
    g = torch.from_numpy(np.random.default_rng(7).normal(size=(len(COUNTS), 3)).astype(np.float32)).to(DEV)

    def run(wanted):
        seg32, leaves = _leaves(seg, sigma, torch.float32)
        for key, leaf in leaves.items():
            leaf.requires_grad_(key in wanted)
        depth, entries = radfoam.ray_quantiles(seg32, leaves["sigma"], quantiles)
        depth.backward(g)
        torch.cuda.synchronize()
        return depth.detach(), entries, leaves

    depth, entries, full = run(KEYS)
    again_depth, again_entries, again = run(KEYS)          # two calls: the same bits, gradients included
    assert torch.equal(depth.view(torch.int32), again_depth.view(torch.int32)) and torch.equal(entries, again_entries)
    for key in KEYS:
        assert not bool(torch.isnan(full[key].grad).any())
        assert torch.equal(full[key].grad.view(torch.int32), again[key].grad.view(torch.int32)), key
    for wanted in [("sigma",), ("t_enter", "t_exit"), ("t_enter",), ("t_exit",), ("sigma", "t_exit")]:
        sub_depth, sub_entries, leaves = run(wanted)
        assert torch.equal(depth.view(torch.int32), sub_depth.view(torch.int32)) and torch.equal(entries, sub_entries)
        for key, leaf in leaves.items():
            if key in wanted:                 # no atomics: the same bits whichever other gradients are computed
                assert torch.equal(leaf.grad.view(torch.int32), full[key].grad.view(torch.int32)), (wanted, key)
            else:
                assert leaf.grad is None, (wanted, key)


def test_more_quantiles_than_the_kernel_takes():
    import radfoam

    most = _max_quantiles()
    seg, sigma = _hand_built([3, 0, 40, 70], seed=9)
    quantiles = _random_quantiles(seg, sigma, most + 1, seed=10)
    _assert_levels_are_clear(seg, sigma, quantiles)
    depth, entries = radfoam.ray_quantiles(seg, sigma.requires_grad_(True), quantiles)      # the torch path
    assert depth.dtype == torch.float32 and depth.shape == (4, most + 1) and "RayQuantiles" not in str(depth.grad_fn)
    ref, ref_entries = radfoam.ray_quantiles(seg, sigma, quantiles, backend="torch")
    assert torch.equal(depth, ref) and torch.equal(entries, ref_entries)
    with pytest.raises(RuntimeError, match="at most %d quantiles" % most):
        radfoam.ray_quantiles(seg, sigma, quantiles, backend="hip")
    hip, _ = radfoam.ray_quantiles(seg, sigma, quantiles[:, :most].contiguous())
    assert "RayQuantiles" in str(hip.grad_fn)


def _device_inputs(fm, rays, starts):
    p, a, adj, off = H.to_torch_foam(fm, DEV)
    r = torch.from_numpy(np.ascontiguousarray(rays)).to(DEV)
    s = torch.from_numpy(np.ascontiguousarray(starts, dtype=np.uint32)).to(DEV)
    return p, a, adj, off, r, s


@pytest.mark.parametrize("weight_threshold", [None, 0.5])
def test_real_walk_against_trace_forward(foam_factory, weight_threshold):
    """pipe.trace_forward(depth_quantiles=q) against ray_quantiles(pipe.trace_segments(...), density[cells], q) under
    the CPU test's criterion: rtol = 1e-6 on the depths (trace_forward works in float32 with a running product, logf
    and a divide), at most 0.5 % of the pairs left out because validity or cell differ, seg["cells"][entries] equal to
    the returned indices elsewhere."""
    import radfoam

    settings = {} if weight_threshold is None else {"weight_threshold": weight_threshold}
    fm, rays, starts, _ = S.image_case(foam_factory, **settings)
    p, a, adj, off, r, s = _device_inputs(fm, rays, starts)
    rng = np.random.default_rng(5)
    q = -np.sort(-rng.uniform(0.02, 0.98, size=rays.shape[:-1] + (3,)).astype(np.float32), axis=-1)
    q = torch.from_numpy(q).to(DEV)
    pipe = radfoam.create_pipeline(2)
    ref = pipe.trace_forward(p, a, adj, off, r, s, depth_quantiles=q, **settings)
    seg = pipe.trace_segments(p, a, adj, off, r, s, **settings)
    cells = seg["cells"].to(torch.int64)
    depth, entries = radfoam.ray_quantiles(seg, a[:, -1].float()[cells].contiguous(), q)
    torch.cuda.synchronize()
    ref_depth = ref["depth"].reshape(-1, 3).double().cpu().numpy()
    ref_cells = ref["depth_indices"].reshape(-1, 3).to(torch.int64).cpu().numpy() & 0xFFFFFFFF
    ref_valid = ref_cells != 0xFFFFFFFF
    valid = (entries >= 0).cpu().numpy()
    got_cells = torch.where(entries >= 0, cells[entries.clamp_min(0)], torch.full_like(entries, 0xFFFFFFFF)).cpu().numpy()
    depth = depth.double().cpu().numpy()
    same = (valid == ref_valid) & (got_cells == ref_cells)
    both = same & valid
    relative = np.abs(depth[both] - ref_depth[both]) / np.abs(ref_depth[both])
    print("weight_threshold %s: %d pairs, %d valid in trace_forward; validity differs on %d, the cell on %d more; "
          "largest depth error %.3g relative, at %.3g of its bound"
          % (weight_threshold, valid.size, ref_valid.sum(), (valid != ref_valid).sum(),
             (~same).sum() - (valid != ref_valid).sum(), relative.max(), relative.max() / 1e-6))
    assert valid.size == 9216 and 0.2 < ref_valid.mean() < 0.8
    assert (~same).mean() <= 0.005
    assert (depth[~valid] == -1).all()
    np.testing.assert_allclose(depth[both], ref_depth[both], rtol=1e-6, atol=0.0)


def test_real_walk_chain_to_points_and_rays(foam_factory):
    """points and rays requiring grad, trace_differentiable_segments, ray_quantiles, the quantile-gap loss, backward:
    against the same chain with backend="torch".  Both chains end in the same atomic kernels, so the criterion is DESIGN
    4.11's for a chain: per element 1e-3 |ref| + 1e-3 rms."""
    import radfoam

    fm, rays, starts, _ = S.image_case(foam_factory)
    density = torch.from_numpy((fm["attributes"][:, -1] + 0.2).astype(np.float32)).to(DEV)
    q = np.random.default_rng(11).uniform(0.02, 0.98, size=(rays.shape[0] * rays.shape[1], 2)).astype(np.float32)
    q = torch.from_numpy(-np.sort(-q, axis=-1)).to(DEV)
    pipe = radfoam.create_pipeline(2)

    def run(**kw):
        p, a, adj, off, r, s = _device_inputs(fm, rays, starts)
        p.requires_grad_(True)
        r.requires_grad_(True)
        seg = pipe.trace_differentiable_segments(p, a, adj, off, r, s)
        assert seg["t_exit"].grad_fn is not None
        depth, entries = radfoam.ray_quantiles(seg, density[seg["cells"].to(torch.int64)], q, **kw)
        both = (entries >= 0).all(dim=-1)
        gap = torch.where(both, (depth[:, 0] - depth[:, 1]).abs(), torch.zeros_like(depth[:, 0]))
        gap.sum().backward()
        torch.cuda.synchronize()
        return entries, gap.detach(), p.grad.cpu().numpy(), r.grad.reshape(-1, 6).cpu().numpy()

    entries, gap, *got = run()
    ref_entries, ref_gap, *want = run(backend="torch")
    agree = (entries == ref_entries).all(dim=-1)
    print("%d of %d rays reach both quantiles; the entries of %d rays differ between the backends; largest gap %.3g"
          % (int((entries >= 0).all(dim=-1).sum()), entries.size(0), int((~agree).sum()), float(ref_gap.max())))
    assert gap.dtype == torch.float32 and float(ref_gap.max()) > 0.1 and int((entries >= 0).all(dim=-1).sum()) > 500
    assert bool(agree.all())                               # float32 gaps of depths near 3: 2.4e-7 each, two of them
    np.testing.assert_allclose(gap.double().cpu().numpy(), ref_gap.double().cpu().numpy(), rtol=2e-7, atol=1e-6)
    for name, g, w in zip(("points.grad", "rays.grad"), got, want):
        assert g.dtype == np.float32 and g.shape == w.shape and np.abs(w).max() > 0
        finite = np.isfinite(w)
        assert np.isfinite(g[finite]).all() and finite.mean() > 0.99
        g, w = g[finite], w[finite]
        ok, rel, worst = H.grad_close(g, w)
        print("%s: relative L2 to the chain through the torch backend %.3g, worst element at %.3g of its bound"
              % (name, rel, worst))
        assert ok, (name, worst)


def test_example_at_toy_size():
    from examples.quantile_regulariser import fit

    plain, regularised, median = fit(num_points=2000, width=32, height=24, steps=10, log=lambda *_: None)
    print("photometric alone: mse %.4g, mean quantile gap %.4g; with the regulariser: mse %.4g, mean quantile gap %.4g"
          % (plain + regularised))
    assert all(np.isfinite(v) for v in plain + regularised)
    assert median.shape == (24, 32) and bool(torch.isfinite(median).all()) and bool((median >= 0).any())
    assert regularised[1] < plain[1]
