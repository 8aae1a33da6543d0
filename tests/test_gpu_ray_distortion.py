"""radfoam.ray_distortion on the GPU (rf_distortion.hip): the kernels against the float64 torch backend on
hand-built lists that put the carry across 64-entry steps, run heads at lane 0 and lane 63, empty rays at a wave's
boundary and a ray longer than a block where they can go wrong, measured in t and in s = t / (1 + t); bitwise
reproducibility; the real walk against the literal |m_i - m_j| double sum; and autograd from the distortion down to
points.grad and rays.grad.

The bar is the project's for a result computed in double and rounded once to float32: rtol = 2e-7, atol = 1e-7 (half
a float32 ulp is 6e-8 relative; both sides read the same float32 inputs)."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import segments_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RTOL, ATOL = 2e-7, 1e-7
COUNTS = [0, 1, 63, 64, 65, 0, 0, 130, 1, 300, 0, 2, 1024]
KEYS = ("sigma", "t_enter", "t_exit", "s_enter", "s_exit")


def _hand_built(counts, seed):
    """The generator of tests/test_gpu_composite_entries.py, restated: per ray a random increasing sequence of times
    with zero-length (t_exit == t_enter) and inverted (t_exit < t_enter) crossings sprinkled in and +inf on some last
    entries; sigma in 0 .. 50 with exact zeros, scaled by 1.2 / n on a ray of n > 1 entries so that the sum of x over a
    ray stays near 2.5 and the last entries of a long ray still carry weight (what a carry gets wrong shows there)."""
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


def _contracted(seg):
    """s = t / (1 + t) in float32: where t_exit is infinite s_exit is nan, on purpose -- the entry has no weight and
    nothing of it may reach the result or a gradient.  Exact ties of t stay exact ties of s."""
    return tuple((t / (1 + t)).contiguous() for t in (seg["t_enter"], seg["t_exit"]))


def _leaves(seg, sigma, s, dtype):
    """Fresh leaves of `dtype` for every differentiable input: (seg, dict of the leaves by name)."""
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)
    leaves = {"sigma": leaf(sigma), "t_enter": leaf(seg["t_enter"]), "t_exit": leaf(seg["t_exit"])}
    if s is not None:
        leaves.update(s_enter=leaf(s[0]), s_exit=leaf(s[1]))
    return {**seg, "t_enter": leaves["t_enter"], "t_exit": leaves["t_exit"]}, leaves


def _call(seg, leaves, **kw):
    import radfoam

    return radfoam.ray_distortion(seg, leaves["sigma"], leaves.get("s_enter"), leaves.get("s_exit"), **kw)


def _close(name, got, want):
    got, want = got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy()
    err = np.abs(got - want)
    bound = ATOL + RTOL * np.abs(want)
    print("%s: largest |kernel - float64 torch backend| %.3g, at %.3g of its bound; largest |reference| %.3g"
          % (name, err.max(initial=0.0), (err / bound).max(initial=0.0), np.abs(want).max(initial=0.0)))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=name)


def _check(name, seg, sigma, s=None, seed=1, g=None):
    """Forward and every gradient for G (random where not given) against float64 autograd of the torch backend.  The
    largest element of every gradient must lie between 0.05 and 1e3."""
    num_rays = seg["offsets"].numel() - 1
    g = np.random.default_rng(seed).normal(size=num_rays) if g is None else np.asarray(g, dtype=np.float64)
    g = torch.from_numpy(g).to(DEV)
    seg32, l32 = _leaves(seg, sigma, s, torch.float32)
    out = _call(seg32, l32)
    assert out.dtype == torch.float32 and out.shape == (num_rays,) and out.is_cuda
    out.backward(g.float())
    seg64, l64 = _leaves(seg, sigma, s, torch.float64)
    ref = _call(seg64, l64, backend="torch")
    assert ref.dtype == torch.float64
    ref.backward(g.float().double())
    torch.cuda.synchronize()
    _close(name + " forward", out, ref)
    assert set(l32) == set(KEYS[:3] if s is None else KEYS)
    for key in l32:
        got, want = l32[key].grad, l64[key].grad
        assert got is not None and got.dtype == torch.float32 and got.shape == want.shape
        # O(1) by construction, so that atol = 1e-7 is a float32 rounding of them and not a free pass
        if want.numel():
            assert 0.05 < float(want.abs().max()) < 1e3, (name, key, float(want.abs().max()))
        _close(name + " grad " + key, got, want)
    infinite = torch.isinf(seg["t_exit"])
    if bool(infinite.any()):
        for key in l32:                                    # exact zeros, and finite whatever s_* hold there
            assert bool((l32[key].grad[infinite] == 0).all()), (name, key)
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(t.grad).all()) for t in l32.values())
    counts = seg["offsets"][1:] - seg["offsets"][:-1]
    assert bool((out[counts == 0] == 0).all())
    return out


@pytest.mark.parametrize("contracted", [False, True])
def test_hand_built_list(contracted):
    seg, sigma = _hand_built(COUNTS, seed=40 + contracted)
    assert bool(torch.isinf(seg["t_exit"]).any()) and bool((seg["t_exit"] == seg["t_enter"]).any())
    assert bool((seg["t_exit"] < seg["t_enter"]).any()) and bool((sigma == 0).any()) and float(sigma.max()) > 20
    s = _contracted(seg) if contracted else None
    assert s is None or bool(torch.isnan(s[1]).any())
    out = _check("hand-built, in %s" % ("s" if contracted else "t"), seg, sigma, s)
    assert int((out > 1e-3).sum()) >= 6


def test_one_ray_and_ray_counts_off_the_wave():
    """R = 1 with one entry; then ray counts that are no multiple of the rays a wave owns, one below and one above a
    multiple, with short rays so that a wave's rays share a step."""
    from radfoam_amd import _lib

    per_wave = int(_lib.load().rf_distortion_rays_per_wave())
    assert 1 <= per_wave <= 63
    # one entry gives one number per gradient.  out = w^2 d / 3; with t = 0.5 .. 2.5 and sigma = 1, w = 0.86 and
    # exp(-x) = 0.14; the smallest gradient is that of the times when d is measured in s (d = 0.38):
    # 2 w d / 3 exp(-x) sigma = 0.03, so G = 4 puts every gradient above 0.05
    seg = {"offsets": torch.tensor([0, 1], device=DEV), "t_enter": torch.tensor([0.5], device=DEV),
           "t_exit": torch.tensor([2.5], device=DEV)}
    sigma = torch.ones(1, device=DEV)
    _check("one ray, one entry", seg, sigma, g=[4.0])
    _check("one ray, one entry, in s", seg, sigma, _contracted(seg), g=[4.0])
    rng = np.random.default_rng(3)
    for num_rays in (5 * per_wave - 1, 4 * per_wave + 1):
        assert num_rays % per_wave != 0
        counts = rng.integers(0, 40, size=num_rays)
        counts[-1] = 7
        seg, sigma = _hand_built(counts, seed=num_rays)
        _check("%d rays" % num_rays, seg, sigma)
        _check("%d rays, in s" % num_rays, seg, sigma, _contracted(seg))


@pytest.mark.parametrize("contracted", [False, True])
def test_needs_input_grad_subsets(contracted):
    seg, sigma = _hand_built(COUNTS, seed=5)
    s = _contracted(seg) if contracted else None
    g = torch.from_numpy(np.random.default_rng(6).normal(size=len(COUNTS)).astype(np.float32)).to(DEV)
    seg32, full = _leaves(seg, sigma, s, torch.float32)
    _call(seg32, full).backward(g)
    subsets = [("sigma",), ("t_enter", "t_exit"), ("t_enter",), ("t_exit",), ("sigma", "t_exit")]
    if contracted:
        subsets += [("s_enter", "s_exit"), ("s_enter",), ("s_exit",), ("sigma", "s_exit"), ("t_enter", "s_enter")]
    for wanted in subsets:
        seg32, leaves = _leaves(seg, sigma, s, torch.float32)
        for key, leaf in leaves.items():
            leaf.requires_grad_(key in wanted)
        _call(seg32, leaves).backward(g)
        torch.cuda.synchronize()
        for key, leaf in leaves.items():
            if key in wanted:                 # no atomics: the same bits whichever other gradients are computed
                assert torch.equal(leaf.grad.view(torch.int32), full[key].grad.view(torch.int32)), (wanted, key)
            else:
                assert leaf.grad is None, (wanted, key)


def test_bitwise_reproducible():
    seg, sigma = _hand_built(COUNTS, seed=7)
    s = _contracted(seg)
    g = torch.from_numpy(np.random.default_rng(8).normal(size=len(COUNTS)).astype(np.float32)).to(DEV)
    for measure in (None, s):
        runs = []
        for _ in range(2):
            seg32, leaves = _leaves(seg, sigma, measure, torch.float32)
            out = _call(seg32, leaves)
            out.backward(g)
            runs.append([out.detach()] + [t.grad for t in leaves.values()])
        torch.cuda.synchronize()
        assert len(runs[0]) == (4 if measure is None else 6)
        for a, b in zip(*runs):
            assert not bool(torch.isnan(a).any()) and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _device_inputs(fm, rays, starts):
    p, a, adj, off = H.to_torch_foam(fm, DEV)
    r = torch.from_numpy(np.ascontiguousarray(rays)).to(DEV)
    s = torch.from_numpy(np.ascontiguousarray(starts, dtype=np.uint32)).to(DEV)
    return p, a, adj, off, r, s


def _double_sum(t_enter, t_exit, sigma):
    """Mip-NeRF 360's sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 d_i of one ray, literally, in float64."""
    n = len(sigma)
    w, m, d, total = np.zeros(n), np.zeros(n), np.zeros(n), 0.0
    for i in range(n):
        infinite = np.isinf(t_exit[i])
        dt = 0.0 if infinite else max(t_exit[i] - t_enter[i], 0.0)
        w[i] = np.exp(-total) * -np.expm1(-sigma[i] * dt)
        total += sigma[i] * dt
        m[i] = 0.0 if infinite else (t_enter[i] + t_exit[i]) / 2
        d[i] = 0.0 if infinite else max(t_exit[i] - t_enter[i], 0.0)
    out = 0.0
    for i in range(n):
        for j in range(n):
            out += w[i] * w[j] * abs(m[i] - m[j])
        out += w[i] * w[i] * d[i] / 3
    return out


def test_real_walk(foam_factory):
    """points and rays requiring grad, trace_differentiable_segments, ray_distortion, .sum().backward(): against the same
    chain with backend="torch".  Both chains end in the same atomic kernels, so the criterion is DESIGN 4.11's for a
    chain: per element 1e-3 |ref| + 1e-3 rms.  And the ordered form IS the distortion loss on a real walk: on the float64
    copy of the walk the forward equals the literal double sum on 32 sampled rays to 1e-9 (relative, plus 1e-9 absolute:
    the float64 backend takes the sums over a ray's earlier entries as differences of cumulative sums over all 78,222
    entries, whose absolute error is 2^-53 times the list-wide sum)."""
    import radfoam

    fm, rays, starts, _ = S.image_case(foam_factory)
    density = torch.from_numpy((fm["attributes"][:, -1] + 0.2).astype(np.float32)).to(DEV)
    pipe = radfoam.create_pipeline(2)

    def run(**kw):
        p, a, adj, off, r, s = _device_inputs(fm, rays, starts)
        p.requires_grad_(True)
        r.requires_grad_(True)
        seg = pipe.trace_differentiable_segments(p, a, adj, off, r, s, weight_threshold=0.5)
        assert seg["t_exit"].grad_fn is not None
        out = radfoam.ray_distortion(seg, density[seg["cells"].to(torch.int64)], **kw)
        out.sum().backward()
        torch.cuda.synchronize()
        return seg, out.detach(), p.grad.cpu().numpy(), r.grad.reshape(-1, 6).cpu().numpy()

    seg, out, *got = run()
    _, ref, *want = run(backend="torch")
    assert out.dtype == torch.float32 and float(ref.max()) > 0.1
    _close("real walk, forward", out, ref.double())
    for name, g, w in zip(("points.grad", "rays.grad"), got, want):
        assert g.dtype == np.float32 and g.shape == w.shape and np.abs(w).max() > 0
        finite = np.isfinite(w)
        assert np.isfinite(g[finite]).all() and finite.mean() > 0.99
        g, w = g[finite], w[finite]
        ok, rel, worst = H.grad_close(g, w)
        print("%s: relative L2 to the chain through the torch backend %.3g, worst element at %.3g of its bound"
              % (name, rel, worst))
        assert ok, (name, worst)

    t_enter, t_exit = seg["t_enter"].detach().double(), seg["t_exit"].detach().double()
    sigma = density[seg["cells"].to(torch.int64)].double()
    out64 = radfoam.ray_distortion({"offsets": seg["offsets"], "t_enter": t_enter, "t_exit": t_exit}, sigma)
    assert out64.dtype == torch.float64
    off, out64 = seg["offsets"].cpu().numpy(), out64.cpu().numpy()
    t_enter, t_exit, sigma = t_enter.cpu().numpy(), t_exit.cpu().numpy(), sigma.cpu().numpy()
    sample = np.random.default_rng(14).choice(len(off) - 1, size=32, replace=False)
    literal = np.array([_double_sum(t_enter[off[r]:off[r + 1]], t_exit[off[r]:off[r + 1]], sigma[off[r]:off[r + 1]])
                        for r in sample])
    print("32 rays: largest |ordered form - double sum| %.3g; double sum %.3g .. %.3g"
          % (np.abs(out64[sample] - literal).max(), literal.min(), literal.max()))
    assert literal.max() > 0.1
    np.testing.assert_allclose(out64[sample], literal, rtol=1e-9, atol=1e-9)


def test_example_at_toy_size():
    from examples.distortion_regulariser import fit

    plain, regularised = fit(num_points=2000, width=32, height=24, steps=10, log=lambda *_: None)
    print("photometric alone: mse %.4g, mean distortion %.4g; with the regulariser: mse %.4g, mean distortion %.4g"
          % (plain + regularised))
    assert all(np.isfinite(v) for v in plain + regularised)
    assert regularised[1] < plain[1]
