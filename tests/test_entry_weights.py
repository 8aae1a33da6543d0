"""CPU: radfoam.entry_weights (torch backend and public surface) on hand-built lists: against a per-ray
float64 loop of the definition and against the hand-written spelling of examples/cell_statistics.py; the identities
that tie it to composite_entries; gradcheck; the gradient formula of DESIGN 4.17 against autograd; validation; the build
lists."""
import os

import numpy as np
import pytest
import torch

import radfoam
import radfoam_amd
from radfoam import entry_weights

# empty rays first, in the middle and last; one-entry rays; at most 70 entries
COUNTS = [0, 1, 5, 0, 0, 70, 33, 2, 7, 1, 12, 3, 9, 21, 4, 6, 0]


def _list(counts, seed, ties=True):
    """A list with the given entries per ray, float64: per ray an increasing sequence of crossings that starts at
    0.2 .. 0.7 with steps of 0.05 .. 0.3; inverted entries (t_exit < t_enter, by 0.05) sprinkled in and, with `ties`,
    zero-length ones (t_exit == t_enter); +inf on the last entry of every odd ray and of the longest; sigma in 0.2 .. 4
    with exact zeros, scaled by 8 / n on a ray of n > 8 entries so that the sum of x over a ray stays near 2.5 and the
    last entries of a long ray still carry weight."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, dtype=np.int64)
    total = int(counts.sum())
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    t_enter, t_exit, sigma = np.zeros(total), np.zeros(total), np.zeros(total)
    for r, n in enumerate(counts):
        if n == 0:
            continue
        e = slice(offsets[r], offsets[r] + n)
        edges = rng.uniform(0.2, 0.7) + np.concatenate([[0.0], np.cumsum(rng.uniform(0.05, 0.3, size=n))])
        t_enter[e], t_exit[e] = edges[:-1], edges[1:]
        kind = rng.uniform(size=n)
        flat, inverted = (kind < 0.1) & ties, (kind >= 0.1) & (kind < 0.2)
        t_exit[e][flat] = t_enter[e][flat]
        t_exit[e][inverted] = t_enter[e][inverted] - 0.05
        if r % 2 == 1 or n == counts.max():
            t_exit[offsets[r] + n - 1] = np.inf
        sigma[e] = rng.uniform(0.2, 4.0, size=n) * (rng.uniform(size=n) > 0.15) * min(1.0, 8.0 / n)
    seg = {"offsets": torch.from_numpy(offsets), "t_enter": torch.from_numpy(t_enter), "t_exit": torch.from_numpy(t_exit)}
    return seg, torch.from_numpy(sigma)


def _case():
    seg, sigma = _list(COUNTS, seed=1)
    assert bool(torch.isinf(seg["t_exit"]).any()) and bool((seg["t_exit"] == seg["t_enter"]).any())
    assert bool((seg["t_exit"] < seg["t_enter"]).any()) and bool((sigma == 0).any())
    return seg, sigma


def _literal(seg, sigma):
    """The definition, ray by ray and entry by entry in float64: (weights [S], transmittance [S])."""
    off, t_enter, t_exit, sigma = seg["offsets"].numpy(), seg["t_enter"].numpy(), seg["t_exit"].numpy(), sigma.numpy()
    weights, through = np.zeros(len(sigma)), np.zeros(len(sigma))
    for r in range(len(off) - 1):
        run = 0.0
        for k in range(off[r], off[r + 1]):
            dt = 0.0 if np.isinf(t_exit[k]) else max(t_exit[k] - t_enter[k], 0.0)
            x = sigma[k] * dt
            through[k] = np.exp(-run)
            weights[k] = through[k] * -np.expm1(-x)
            run += x
    return weights, through


def _leaves(seg, sigma):
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    t0, t1, sig = leaf(seg["t_enter"]), leaf(seg["t_exit"]), leaf(sigma)
    return {**seg, "t_enter": t0, "t_exit": t1}, sig


def _entry_rays(seg):
    off = seg["offsets"]
    return torch.repeat_interleave(torch.arange(off.numel() - 1), off[1:] - off[:-1])


def test_public_surface():
    assert "entry_weights" in radfoam_amd.__all__ and "entry_weights" in radfoam.__all__
    assert radfoam.entry_weights is radfoam_amd.segments.entry_weights


def test_sources_are_built_but_not_part_of_the_source_hash():
    from radfoam_amd import _lib, build

    names = lambda paths: {os.path.basename(p) for p in paths}
    assert "rf_entry_weights.hip" in names(build.EXTRA_SOURCES)
    assert {"radfoam_hip_entry_weights.h", "rf_ray_sweep.hpp"} <= names(build.EXTRA_HEADERS)
    assert not names(build.SOURCES + build.HEADERS) & {"rf_entry_weights.hip", "radfoam_hip_entry_weights.h"}
    assert not names(build.SOURCES + build.HEADERS) & names(build.EXTRA_SOURCES + build.EXTRA_HEADERS)
    for path in build.EXTRA_SOURCES + build.EXTRA_HEADERS:
        assert os.path.exists(path), path
    lib = _lib.load()
    for name in ("rf_entry_weights_forward", "rf_entry_weights_backward", "rf_entry_weights_rays_per_wave"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert 1 <= lib.rf_entry_weights_rays_per_wave() <= 63
    # nothing to do: no rays, or no entries
    assert lib.rf_entry_weights_forward(0, None, 0, None, None, None, None, None, None) == 0
    assert lib.rf_entry_weights_forward(5, None, 0, None, None, None, None, None, None) == 0
    assert lib.rf_entry_weights_backward(0, None, 0, None, None, None, None, None, None, None, None, None) == 0
    dummy = np.zeros(64).ctypes.data
    assert lib.rf_entry_weights_forward(5, dummy, 3, dummy, dummy, dummy, None, dummy, None) == -1   # weights is required
    assert "null pointer" in _lib.last_error()
    assert lib.rf_entry_weights_forward(5, None, 3, dummy, dummy, dummy, dummy, None, None) == -1
    assert "null pointer" in _lib.last_error()
    assert lib.rf_entry_weights_forward(5, dummy, -1, dummy, dummy, dummy, dummy, dummy, None) == -1
    assert "negative entry count" in _lib.last_error()
    assert lib.rf_entry_weights_backward(5, dummy, -1, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy,
                                         None) == -1
    assert "negative entry count" in _lib.last_error()
    assert lib.rf_entry_weights_backward(5, dummy, 3, dummy, dummy, None, dummy, None, dummy, None, None, None) == -1
    assert "null pointer" in _lib.last_error()
    # no gradient asked for: nothing to do, whatever else is missing
    assert lib.rf_entry_weights_backward(5, None, 3, None, None, None, None, None, None, None, None, None) == 0


def test_matches_the_literal_loop():
    """rtol = 1e-12 with no atol: the restatement takes the sum in front of an entry as a difference of two values of
    one list-wide cumulative sum, an absolute error of about 2^-53 times that sum (40 here) in the exponent, 5e-15
    relative in T and w."""
    seg, sigma = _case()
    want_w, want_t = _literal(seg, sigma)
    weights, through = entry_weights(seg, sigma, return_transmittance=True)
    assert weights.dtype == torch.float64 and weights.shape == sigma.shape and through.shape == sigma.shape
    assert float(want_w.max()) > 0.3 and float(want_t.min()) < 0.2
    np.testing.assert_allclose(weights.numpy(), want_w, rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(through.numpy(), want_t, rtol=1e-12, atol=0.0)
    alone = entry_weights(seg, sigma)
    assert isinstance(alone, torch.Tensor) and torch.equal(alone, weights)
    assert torch.equal(entry_weights(seg, sigma, backend="torch"), weights)


def test_matches_the_example_spelling():
    from examples.cell_statistics import entry_weights as by_hand

    seg, sigma = _case()
    want, ray = by_hand(seg, sigma)
    assert torch.equal(ray, _entry_rays(seg))
    np.testing.assert_allclose(entry_weights(seg, sigma).numpy(), want.numpy(), rtol=1e-12, atol=0.0)


def test_identities():
    seg, sigma = _case()
    weights, through = entry_weights(seg, sigma, return_transmittance=True)
    off, ray = seg["offsets"], _entry_rays(seg)
    counts = off[1:] - off[:-1]
    assert bool((through[off[:-1][counts > 0]] == 1).all())                       # exactly 1 at every ray's first entry
    inner = torch.ones(sigma.numel(), dtype=torch.bool)
    inner[off[1:][counts > 0] - 1] = False                                        # entries with a successor in their ray
    at = torch.nonzero(inner).reshape(-1)
    assert at.numel() == sigma.numel() - int((counts > 0).sum())
    assert float(((through - weights)[at] - through[at + 1]).abs().max()) <= 1e-14
    infinite = torch.isinf(seg["t_exit"])
    assert int(infinite.sum()) >= 3 and bool((weights[infinite] == 0).all())

    channels = 3
    values = torch.from_numpy(np.random.default_rng(2).uniform(-1.0, 1.0, size=(sigma.numel(), channels)))
    composited = radfoam.composite_entries(seg, sigma, values, backend="torch")
    num_rays = len(COUNTS)
    per_ray = torch.zeros(num_rays, dtype=torch.float64).index_add(0, ray, weights)
    np.testing.assert_allclose(per_ray.numpy(), composited[:, channels].numpy(), rtol=1e-12, atol=1e-12)
    summed = torch.zeros((num_rays, channels), dtype=torch.float64).index_add(0, ray, weights.unsqueeze(-1) * values)
    np.testing.assert_allclose(summed.numpy(), composited[:, :channels].numpy(), rtol=1e-12, atol=1e-12)


def test_gradcheck():
    """Crossings strictly positive, strictly inverted by 0.05, or infinite: none at t_exit == t_enter, where clamp_min
    has a kink."""
    seg, sigma = _list([0, 1, 5, 0, 9], seed=2, ties=False)
    assert not bool((seg["t_exit"] == seg["t_enter"]).any())
    assert bool(torch.isinf(seg["t_exit"]).any()) and bool((seg["t_exit"] < seg["t_enter"]).any())
    infinite = torch.isinf(seg["t_exit"])
    fn = lambda sig, t0, t1: entry_weights({**seg, "t_enter": t0, "t_exit": t1}, sig, return_transmittance=True)
    inputs = tuple(t.clone().requires_grad_(True) for t in (sigma, seg["t_enter"], seg["t_exit"]))
    assert torch.autograd.gradcheck(fn, inputs, eps=1e-6, atol=1e-7, rtol=1e-5)
    assert torch.autograd.gradcheck(lambda *a: fn(*a)[0], inputs, eps=1e-6, atol=1e-7, rtol=1e-5)
    weights, through = fn(*inputs)
    (weights.sum() + 2 * through.sum()).backward()
    for t in inputs:                                       # behind an infinite t_exit: exact zeros, selected
        assert bool((t.grad[infinite] == 0).all()) and float(t.grad.abs().max()) > 1e-2


def _closed_form(seg, sigma, g_w, g_t):
    """DESIGN 4.17's formulas in a few lines of float64 torch: grad_sigma, grad_t_enter, grad_t_exit."""
    off, ray = seg["offsets"], _entry_rays(seg)
    t_enter, t_exit = seg["t_enter"], seg["t_exit"]
    infinite = torch.isinf(t_exit)
    dt = torch.where(infinite, torch.zeros_like(t_exit), (t_exit - t_enter).clamp_min(0.0))
    x = sigma * dt
    run = torch.cat([x.new_zeros(1), torch.cumsum(x, 0)])
    through = torch.exp(-(run[:-1] - run[off[:-1]][ray]))
    weights = through * -torch.expm1(-x)
    u = g_w * weights + g_t * through
    upto = torch.cumsum(u, 0)                                                     # inclusive, over the whole list
    later = torch.cat([u.new_zeros(1), upto])[off[1:]][ray] - upto                # over the ray's later entries
    dx = g_w * through * torch.exp(-x) - later
    moves = ~infinite & (t_exit >= t_enter)
    g_exit = torch.where(moves, dx * sigma, torch.zeros_like(dx))
    return torch.where(infinite, torch.zeros_like(dx), dx * dt), -g_exit, g_exit


def test_closed_form():
    """DESIGN 4.17's gradient formulas equal autograd to 1e-10 on the list with ties, inverted crossings, infinite exits
    and exact-zero densities; entries behind an infinite t_exit get exact zeros."""
    seg, sigma = _case()
    rng = np.random.default_rng(3)
    g_w, g_t = (torch.from_numpy(rng.normal(size=sigma.numel())) for _ in range(2))
    seg_l, sigma_l = _leaves(seg, sigma)
    weights, through = entry_weights(seg_l, sigma_l, return_transmittance=True)
    torch.autograd.backward([weights, through], [g_w, g_t])
    want = _closed_form(seg, sigma, g_w, g_t)
    for got, w in zip((sigma_l.grad, seg_l["t_enter"].grad, seg_l["t_exit"].grad), want):
        assert float(w.abs().max()) > 0.5
        np.testing.assert_allclose(got.numpy(), w.numpy(), rtol=1e-10, atol=1e-10)
    infinite = torch.isinf(seg["t_exit"])
    for t in (sigma_l, seg_l["t_enter"], seg_l["t_exit"]):
        assert bool((t.grad[infinite] == 0).all())
    inverted = seg["t_exit"] < seg["t_enter"]
    assert bool((seg_l["t_exit"].grad[inverted] == 0).all()) and bool((seg_l["t_enter"].grad[inverted] == 0).all())
    ties = seg["t_exit"] == seg["t_enter"]                                        # clamp_min: equality passes it on
    assert float(seg_l["t_exit"].grad[ties].abs().max()) > 1e-3


def test_empty_batch_and_rays_without_entries():
    none = {"offsets": torch.zeros(1, dtype=torch.int64), "t_exit": torch.zeros(0), "t_enter": torch.zeros(0)}
    weights, through = entry_weights(none, torch.zeros(0, dtype=torch.float64), return_transmittance=True)
    assert weights.shape == (0,) and through.shape == (0,) and weights.dtype == torch.float64
    only_empty = {"offsets": torch.zeros(4, dtype=torch.int64), "t_exit": torch.zeros(0), "t_enter": torch.zeros(0)}
    weights = entry_weights(only_empty, torch.zeros(0))
    assert weights.shape == (0,) and weights.dtype == torch.float32


def test_validation():
    seg = {"offsets": torch.tensor([0, 2, 3]), "t_exit": torch.tensor([1.0, 2.0, 0.5]),
           "t_enter": torch.tensor([0.0, 1.0, 0.0])}
    sigma = torch.rand(3)
    weights, through = entry_weights(seg, sigma, return_transmittance=True)
    assert weights.dtype == torch.float32 and through.dtype == torch.float32 and weights.shape == (3,)
    want = entry_weights({k: v.double() if v.is_floating_point() else v for k, v in seg.items()}, sigma.double())
    np.testing.assert_allclose(weights.numpy(), want.numpy(), rtol=2e-7, atol=1e-7)
    for backend in ("cuda", "HIP", ""):
        with pytest.raises(ValueError, match="backend must be None, 'hip' or 'torch'"):
            entry_weights(seg, sigma, backend=backend)
    bad = [
        ((seg, sigma.to(torch.float16)), "sigma must have float32 or float64 dtype"),
        ((seg, sigma.to(torch.int64)), "sigma must have float32 or float64 dtype"),
        ((seg, sigma.reshape(3, 1)), r"expected sigma \[S\]"),
        ((seg, sigma[0]), r"expected sigma \[S\]"),
        ((seg, sigma[:2]), "one element per entry"),
        (({**seg, "t_enter": seg["t_enter"][:2]}, sigma), "one element per entry"),
        (({**seg, "t_exit": seg["t_exit"][:2]}, sigma), "one element per entry"),
        (({**seg, "offsets": seg["offsets"].to(torch.int32)}, sigma), r"seg\['offsets'\] must be int64"),
        (({**seg, "offsets": seg["offsets"].reshape(1, 3)}, sigma), r"seg\['offsets'\] must be int64"),
        (({**seg, "offsets": torch.tensor([0, 2, 2])}, sigma), r"seg\['offsets'\]\[-1\] must be the number"),
    ]
    for args, message in bad:
        with pytest.raises(RuntimeError, match=message):
            entry_weights(*args)
    with pytest.raises(RuntimeError, match="the kernel takes float32 CUDA sigma"):
        entry_weights(seg, sigma, backend="hip")
