"""CPU: radfoam.ray_quantiles (torch backend and public surface) on hand-built lists: against a per-ray
float64 loop of the definition (which restates the reference's `while`), the conventions for quantiles at and outside
0 .. 1, its gradients against finite differences, against the closed form of DESIGN 4.14 in a float64 loop and, on exact
ties, against autograd through a clamp_min restatement; against the oracle's trace_forward(depth_quantiles=...) on a
real walk; validation; the build lists."""
import os

import numpy as np
import pytest
import torch

import radfoam
import radfoam_amd
from radfoam import ray_quantiles
from tests import segments_ref as S

# empty rays first, in the middle and last; at most 70 entries
COUNTS = [0, 1, 5, 0, 0, 70, 33, 2, 7, 0, 12, 3, 9, 21, 4, 6, 0]


def _list(counts, seed, ties=True):
    """A list with the given entries per ray, float64: per ray an increasing sequence of crossings that starts at
    0.2 .. 0.7 with steps of 0.05 .. 0.3; inverted entries (t_exit < t_enter) sprinkled in and, with `ties`, zero-length
    ones (t_exit == t_enter); +inf on the last entry of every odd ray and of the longest; sigma in 0.2 .. 4 with exact
    zeros, scaled by 8 / n on a ray of n > 8 entries so that the sum of x over a ray stays near 2.5; the first two
    entries of every ray of five or more have density 0: zeros in front of the first weight."""
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
        if n >= 5:
            sigma[offsets[r]:offsets[r] + 2] = 0.0
    seg = {"offsets": torch.from_numpy(offsets), "t_enter": torch.from_numpy(t_enter), "t_exit": torch.from_numpy(t_exit)}
    return seg, torch.from_numpy(sigma)


def _x(t_enter, t_exit, sigma):
    dt = np.where(np.isinf(t_exit), 0.0, np.maximum(t_exit - t_enter, 0.0))
    return sigma * dt


def _totals(seg, sigma):
    """[R]: the sum of x over every ray, entry by entry."""
    off = seg["offsets"].numpy()
    x = _x(seg["t_enter"].numpy(), seg["t_exit"].numpy(), sigma.numpy())
    out = np.zeros(len(off) - 1)
    for r in range(len(off) - 1):
        for k in range(off[r], off[r + 1]):
            out[r] += x[k]
    return out


def _level(q):
    """L of the definition for one quantile."""
    if np.isnan(q) or q <= 0:
        return np.inf
    return max(-np.log(q), 0.0)


def _literal(seg, sigma, quantiles):
    """The definition, ray by ray and quantile by quantile in float64: (depth [R, Q], entries [R, Q], X at the crossing)."""
    off, t_enter, t_exit, sigma = seg["offsets"].numpy(), seg["t_enter"].numpy(), seg["t_exit"].numpy(), sigma.numpy()
    quantiles = np.asarray(quantiles, dtype=np.float64).reshape(len(off) - 1, -1)
    depth, entries = np.full(quantiles.shape, -1.0), np.full(quantiles.shape, -1, dtype=np.int64)
    before = np.zeros(quantiles.shape)
    for r in range(len(off) - 1):
        for q in range(quantiles.shape[1]):
            level, run = _level(quantiles[r, q]), 0.0
            for k in range(off[r], off[r + 1]):
                dt = 0.0 if np.isinf(t_exit[k]) else max(t_exit[k] - t_enter[k], 0.0)
                upto = run + sigma[k] * dt
                if upto > level:                       # the reference's next_transmittance < quantile
                    depth[r, q] = t_enter[k] + (level - run) / sigma[k]          # t_0 + log(T / q) / s
                    entries[r, q], before[r, q] = k, run
                    break
                run = upto
    return depth, entries, before


def _quantiles(seg, sigma, num_q, seed, sort=False):
    """[R, Q] float64: exp(-u X_total) of the ray's own total with u in 0 .. 1.3, so that about a quarter is never
    reached; in random order, or sorted descending as train.py's."""
    rng = np.random.default_rng(seed)
    totals = _totals(seg, sigma)
    q = np.exp(-rng.uniform(0.0, 1.3, size=(len(totals), num_q)) * np.maximum(totals, 0.5)[:, None])
    if sort:
        q = -np.sort(-q, axis=-1)
    return torch.from_numpy(q)


def _leaves(seg, sigma):
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    t0, t1, sig = leaf(seg["t_enter"]), leaf(seg["t_exit"]), leaf(sigma)
    return {**seg, "t_enter": t0, "t_exit": t1}, sig


def test_public_surface():
    assert "ray_quantiles" in radfoam_amd.__all__ and "ray_quantiles" in radfoam.__all__
    assert radfoam.ray_quantiles is radfoam_amd.segments.ray_quantiles


def test_sources_are_built_but_not_part_of_the_source_hash():
    from radfoam_amd import _lib, build

    names = lambda paths: {os.path.basename(p) for p in paths}
    assert "rf_quantiles.hip" in names(build.EXTRA_SOURCES)
    assert {"radfoam_hip_quantiles.h", "rf_ray_sweep.hpp"} <= names(build.EXTRA_HEADERS)
    assert not names(build.SOURCES + build.HEADERS) & {"rf_quantiles.hip", "radfoam_hip_quantiles.h"}
    assert not names(build.SOURCES + build.HEADERS) & names(build.EXTRA_SOURCES + build.EXTRA_HEADERS)
    lib = _lib.load()
    for name in ("rf_ray_quantiles_forward", "rf_ray_quantiles_backward", "rf_quantiles_rays_per_wave",
                 "rf_quantiles_max"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert 1 <= lib.rf_quantiles_rays_per_wave() <= 63 and 2 <= lib.rf_quantiles_max() <= 32
    most = lib.rf_quantiles_max()
    assert lib.rf_ray_quantiles_forward(0, None, 0, None, None, None, 2, None, None, None, None) == 0    # nothing to do
    assert lib.rf_ray_quantiles_backward(0, None, 0, None, None, None, 2, None, None, None, None, None, None, None) == 0
    dummy = np.zeros(64).ctypes.data
    assert lib.rf_ray_quantiles_forward(5, None, 3, None, None, None, 2, None, dummy, dummy, None) == -1
    assert "null pointer" in _lib.last_error()
    assert lib.rf_ray_quantiles_forward(5, dummy, 3, dummy, dummy, dummy, 2, None, dummy, dummy, None) == -1
    assert "null pointer" in _lib.last_error()
    assert lib.rf_ray_quantiles_forward(5, dummy, 3, dummy, dummy, dummy, 2, dummy, dummy, None, None) == -1
    assert "null pointer" in _lib.last_error()
    for bad in (0, most + 1):
        assert lib.rf_ray_quantiles_forward(5, dummy, 3, dummy, dummy, dummy, bad, dummy, dummy, dummy, None) == -1
        assert "number of quantiles" in _lib.last_error()
    assert lib.rf_ray_quantiles_forward(5, dummy, -1, dummy, dummy, dummy, 2, dummy, dummy, dummy, None) == -1
    assert "negative entry count" in _lib.last_error()
    assert lib.rf_ray_quantiles_backward(5, None, 3, None, None, None, 2, None, None, None, dummy, None, None, None) == -1
    assert "null pointer" in _lib.last_error()
    assert lib.rf_ray_quantiles_backward(5, dummy, 3, dummy, dummy, dummy, 2, dummy, None, dummy, dummy, None, None,
                                         None) == -1
    assert "null pointer" in _lib.last_error()
    assert lib.rf_ray_quantiles_backward(5, dummy, 3, dummy, dummy, dummy, most + 1, dummy, dummy, dummy, dummy, None,
                                         None, None) == -1
    assert "number of quantiles" in _lib.last_error()
    # no gradient asked for: nothing to do, whatever else is missing
    assert lib.rf_ray_quantiles_backward(5, None, 3, None, None, None, 2, None, None, None, None, None, None, None) == 0


@pytest.mark.parametrize("num_q", [1, 2, 3, 9])
@pytest.mark.parametrize("sort", [False, True])
def test_matches_the_literal_loop(num_q, sort):
    """rtol = 1e-12 with no atol, entries equal.  The restatement takes X_j as a difference of two values of one
    list-wide cumulative sum, so it carries an absolute error of about 2^-53 times that sum (30 here): 3e-15, which the
    division by sigma[j] >= 0.02 turns into 2e-13 at the most, against depths of 0.2 and more."""
    seg, sigma = _list(COUNTS, seed=1)
    assert bool(torch.isinf(seg["t_exit"]).any()) and bool((seg["t_exit"] == seg["t_enter"]).any())
    assert bool((seg["t_exit"] < seg["t_enter"]).any()) and bool((sigma == 0).any())
    off = seg["offsets"].tolist()
    assert all(float(sigma[off[r]:off[r] + 2].abs().max()) == 0 for r in (2, 5, 6, 8, 10, 12, 13, 15))
    quantiles = _quantiles(seg, sigma, num_q, seed=10 + num_q, sort=sort)
    want_depth, want_entries, _ = _literal(seg, sigma, quantiles)
    depth, entries = ray_quantiles(seg, sigma, quantiles)
    assert depth.dtype == torch.float64 and depth.shape == (len(COUNTS), num_q)
    assert entries.dtype == torch.int64 and entries.shape == (len(COUNTS), num_q) and not entries.requires_grad
    counts = np.asarray(COUNTS)
    assert (entries.numpy()[counts == 0] == -1).all() and (depth.numpy()[counts == 0] == -1).all()
    found = want_entries >= 0
    print("Q = %d: %d of %d pairs cross; largest relative difference %.3g"
          % (num_q, found.sum(), found.size,
             np.abs(depth.numpy() / want_depth - 1)[found].max(initial=0.0)))
    assert num_q * 2 <= found.sum() < found.size and want_depth[found].min() >= 0.2
    assert (entries.numpy() == want_entries).all()
    assert (depth.numpy()[~found] == -1).all()
    np.testing.assert_allclose(depth.numpy(), want_depth, rtol=1e-12, atol=0.0)
    # any shape with R Q elements whose last dimension is Q
    again, _ = ray_quantiles(seg, sigma, quantiles.reshape(1, len(COUNTS), num_q))
    assert again.shape == (len(COUNTS), num_q) and torch.equal(again, depth)
    # float32 inputs: the same to a float32 rounding of the result, on the entries the widened inputs give
    seg32 = {**seg, "t_enter": seg["t_enter"].float(), "t_exit": seg["t_exit"].float()}
    got32, entries32 = ray_quantiles(seg32, sigma.float(), quantiles.float(), backend="torch")
    assert got32.dtype == torch.float32 and entries32.dtype == torch.int64
    seg64 = {**seg, "t_enter": seg32["t_enter"].double(), "t_exit": seg32["t_exit"].double()}
    want32, want_entries32 = ray_quantiles(seg64, sigma.float().double(), quantiles.float().double())
    assert torch.equal(entries32, want_entries32)
    np.testing.assert_allclose(got32.numpy(), want32.numpy(), rtol=2e-7, atol=1e-7)


def test_empty_batch_and_rays_without_entries():
    none = {"offsets": torch.zeros(1, dtype=torch.int64), "t_exit": torch.zeros(0), "t_enter": torch.zeros(0)}
    depth, entries = ray_quantiles(none, torch.zeros(0, dtype=torch.float64), torch.zeros((0, 2), dtype=torch.float64))
    assert depth.shape == (0, 2) and depth.dtype == torch.float64 and entries.shape == (0, 2)
    assert entries.dtype == torch.int64
    only_empty = {"offsets": torch.zeros(4, dtype=torch.int64), "t_exit": torch.zeros(0), "t_enter": torch.zeros(0)}
    depth, entries = ray_quantiles(only_empty, torch.zeros(0), torch.full((3, 2), 0.5))
    assert depth.shape == (3, 2) and depth.dtype == torch.float32 and bool((depth == -1).all())
    assert entries.shape == (3, 2) and bool((entries == -1).all())
    # one entry behind an infinite t_exit alone: no weight, nothing is reached, zero gradients
    seg = {"offsets": torch.tensor([0, 1]), "t_enter": torch.tensor([0.5], dtype=torch.float64, requires_grad=True),
           "t_exit": torch.tensor([float("inf")], dtype=torch.float64, requires_grad=True)}
    sigma = torch.tensor([2.0], dtype=torch.float64, requires_grad=True)
    depth, entries = ray_quantiles(seg, sigma, torch.tensor([[0.5, 1.0]], dtype=torch.float64))
    depth.sum().backward()
    assert depth.tolist() == [[-1.0, -1.0]] and entries.tolist() == [[-1, -1]]
    assert float(sigma.grad) == 0 and float(seg["t_enter"].grad) == 0 and float(seg["t_exit"].grad) == 0


def test_quantile_conventions():
    """One ray: two entries without density, then x = 1 over 1 .. 1.5, a zero-length entry, x = 1 over 1.5 .. 2.5."""
    seg = {"offsets": torch.tensor([0, 5]), "t_enter": torch.tensor([0.0, 0.25, 1.0, 1.5, 1.5], dtype=torch.float64),
           "t_exit": torch.tensor([0.25, 1.0, 1.5, 1.5, 2.5], dtype=torch.float64)}
    sigma = torch.tensor([0.0, 0.0, 2.0, 7.0, 1.0], dtype=torch.float64)
    final = float(np.exp(-2.0))

    def one(q):
        depth, entries = ray_quantiles(seg, sigma, torch.tensor([[q]], dtype=torch.float64))
        return float(depth), int(entries)

    assert one(1.0) == (1.0, 2) and one(1.5) == (1.0, 2) and one(float("inf")) == (1.0, 2)     # >= 1 behaves as 1
    assert one(0.0) == (-1.0, -1) and one(-0.3) == (-1.0, -1) and one(float("nan")) == (-1.0, -1)
    assert one(final * 0.999) == (-1.0, -1)                # below the ray's final transmittance
    depth, entry = one(final * 1.001)
    assert entry == 4 and 2.49 < depth < 2.5
    depth, entry = one(float(np.exp(-0.5)))
    assert entry == 2 and abs(depth - 1.25) < 1e-15
    depth, entry = one(float(np.exp(-1.5)))
    assert entry == 4 and abs(depth - 2.0) < 1e-15
    # an unsorted row equals the same quantiles evaluated one at a time
    row = [0.2, 0.9, float("nan"), 0.5, 1.0, 0.1, 0.0, 0.7, 0.3]
    depth, entries = ray_quantiles(seg, sigma, torch.tensor([row], dtype=torch.float64))
    singles = [one(q) for q in row]
    assert depth[0].tolist() == [d for d, _ in singles] and entries[0].tolist() == [e for _, e in singles]
    assert sum(e >= 0 for _, e in singles) == 6


def _inside(seg, sigma, num_q, seed, low=0.2, high=0.8):
    """[R, Q] float64 quantiles whose levels lie well inside an entry: L = X_j + u x_j for a random entry j of the ray
    with x_j > 0 and u in low .. high; a quantile that is never reached for a ray without such an entry."""
    rng = np.random.default_rng(seed)
    off = seg["offsets"].numpy()
    x = _x(seg["t_enter"].numpy(), seg["t_exit"].numpy(), sigma.numpy())
    q = np.full((len(off) - 1, num_q), 1e-30)
    for r in range(len(off) - 1):
        run = np.concatenate([[0.0], np.cumsum(x[off[r]:off[r + 1]])])
        carrying = np.nonzero(x[off[r]:off[r + 1]] > 0)[0]
        if len(carrying):
            j = rng.choice(carrying, size=num_q)
            q[r] = np.exp(-(run[j] + rng.uniform(low, high, size=num_q) * x[off[r]:off[r + 1]][j]))
    return torch.from_numpy(q)


def _gradcheck_case():
    counts = [3, 0, 7, 5, 1, 9, 4, 6, 0, 2, 8, 5, 3, 7, 1, 6, 4, 12, 5, 3]
    seg, sigma = _list(counts, seed=2, ties=False)
    assert len(counts) == 20 and not bool((seg["t_exit"] == seg["t_enter"]).any())
    assert bool(torch.isinf(seg["t_exit"]).any()) and bool((seg["t_exit"] < seg["t_enter"]).any())
    return seg, sigma


def test_gradcheck():
    seg, sigma = _gradcheck_case()
    quantiles = _inside(seg, sigma, 2, seed=3)
    infinite = torch.isinf(seg["t_exit"])
    fn = lambda sig, t0, t1: ray_quantiles({**seg, "t_enter": t0, "t_exit": t1}, sig, quantiles)[0]
    inputs = tuple(t.clone().requires_grad_(True) for t in (sigma, seg["t_enter"], seg["t_exit"]))
    assert int((fn(*inputs) >= 0).sum()) >= 30
    assert torch.autograd.gradcheck(fn, inputs, eps=1e-6, atol=1e-7, rtol=1e-5)
    fn(*inputs).sum().backward()
    for t in inputs:                                       # behind an infinite t_exit: exact zeros, selected
        assert bool((t.grad[infinite] == 0).all()) and float(t.grad.abs().max()) > 1e-3
    q_leaf = quantiles.clone().requires_grad_(True)        # not differentiable in the quantiles
    depth, entries = ray_quantiles(seg, inputs[0], q_leaf)
    assert not entries.requires_grad
    depth.sum().backward()
    assert q_leaf.grad is None


def _closed_form(seg, sigma, quantiles, entries, grad):
    """DESIGN 4.14's formulas in a float64 loop: grad_sigma, grad_t_enter, grad_t_exit."""
    off, t_enter, t_exit, sigma = seg["offsets"].numpy(), seg["t_enter"].numpy(), seg["t_exit"].numpy(), sigma.numpy()
    g_sigma, g_enter, g_exit = np.zeros(len(sigma)), np.zeros(len(sigma)), np.zeros(len(sigma))
    for r in range(len(off) - 1):
        run = 0.0
        for k in range(off[r], off[r + 1]):
            infinite = np.isinf(t_exit[k])
            dt = 0.0 if infinite else max(t_exit[k] - t_enter[k], 0.0)
            passes = not infinite and t_exit[k] >= t_enter[k]
            later = own_sigma = own_enter = 0.0
            for q in range(quantiles.shape[1]):
                j = entries[r, q]
                if j > k:
                    later += grad[r, q] / sigma[j]
                elif j == k:
                    own_sigma += grad[r, q] / sigma[k] * (_level(quantiles[r, q]) - run) / sigma[k]
                    own_enter += grad[r, q]
            if not infinite:
                g_sigma[k] = -dt * later - own_sigma
                g_enter[k] = (sigma[k] * later if passes else 0.0) + own_enter
                g_exit[k] = -sigma[k] * later if passes else 0.0
            run += sigma[k] * dt
    return g_sigma, g_enter, g_exit


@pytest.mark.parametrize("ties", [False, True])
def test_closed_form(ties):
    """DESIGN 4.14's gradient formulas, with every sum written out, equal autograd to 1e-10; entries behind an infinite
    t_exit get exact zeros."""
    seg, sigma = _list(COUNTS, seed=3) if ties else _gradcheck_case()
    assert bool((seg["t_exit"] == seg["t_enter"]).any()) == ties
    quantiles = _quantiles(seg, sigma, 3, seed=4)
    num_rays = seg["offsets"].numel() - 1
    grad = np.random.default_rng(5).normal(size=(num_rays, 3))
    seg_l, sigma_l = _leaves(seg, sigma)
    depth, entries = ray_quantiles(seg_l, sigma_l, quantiles)
    depth.backward(torch.from_numpy(grad))
    assert int((entries >= 0).sum()) >= 10 and int((entries < 0).sum()) >= 3
    g_sigma, g_enter, g_exit = _closed_form(seg, sigma, quantiles.numpy(), entries.numpy(), grad)
    close = lambda got, want: np.testing.assert_allclose(got.numpy(), want, rtol=1e-10, atol=1e-10)
    close(sigma_l.grad, g_sigma)
    close(seg_l["t_enter"].grad, g_enter)
    close(seg_l["t_exit"].grad, g_exit)
    assert float(sigma_l.grad.abs().max()) > 1e-2 and np.abs(g_exit).max() > 1e-2
    infinite = torch.isinf(seg["t_exit"])
    assert int(infinite.sum()) >= 3
    for t in (sigma_l, seg_l["t_enter"], seg_l["t_exit"]):
        assert bool((t.grad[infinite] == 0).all())
    # t_exit of an entry nothing crosses behind gets nothing (autograd's reverse cumulative sum leaves 1e-16 there)
    last_only = torch.ones_like(infinite)
    for r in range(num_rays):
        js = entries[r][entries[r] >= 0]
        if len(js):
            last_only[seg["offsets"][r]:int(js.max())] = False
    assert int(last_only.sum()) >= 20 and float(seg_l["t_exit"].grad[last_only].abs().max()) < 1e-12
    assert (g_exit[last_only.numpy()] == 0).all()


def test_tie_convention_is_clamp_min():
    """On a list with exact ties (t_exit == t_enter) the gradients equal autograd through a restatement, ray by ray
    with torch operations, in which max(., 0) is clamp_min and the crossing entries are the ones ray_quantiles found: a
    tied entry in front of a crossing passes sigma c on to its two times."""
    seg, sigma = _list(COUNTS, seed=5)
    ties = seg["t_exit"] == seg["t_enter"]
    assert int(ties.sum()) >= 5
    quantiles = _inside(seg, sigma, 3, seed=6, low=0.6, high=0.9)
    grad = torch.from_numpy(np.random.default_rng(7).normal(size=(len(COUNTS), 3)))
    seg_l, sigma_l = _leaves(seg, sigma)
    depth, entries = ray_quantiles(seg_l, sigma_l, quantiles)
    depth.backward(grad)
    levels = torch.from_numpy(np.vectorize(_level)(quantiles.numpy()))

    seg_r, sigma_r = _leaves(seg, sigma)
    off, rows = seg["offsets"].tolist(), []
    for r in range(len(COUNTS)):
        e = slice(off[r], off[r + 1])
        t0, t1, sig = seg_r["t_enter"][e], seg_r["t_exit"][e], sigma_r[e]
        finite = torch.isfinite(t1.detach())
        x = torch.where(finite, sig * (torch.where(finite, t1, t0) - t0).clamp_min(0.0), torch.zeros_like(sig))
        before = torch.cumsum(x, 0) - x
        for q in range(3):
            j = int(entries[r, q]) - off[r]
            rows.append(grad[r, q] * (t0[j] + (levels[r, q] - before[j]) / sig[j]) if j >= 0 else grad[r, q] * 0)
    torch.stack(rows).sum().backward()
    for got, want, at in ((sigma_l, sigma_r, None), (seg_l["t_enter"], seg_r["t_enter"], ties),
                          (seg_l["t_exit"], seg_r["t_exit"], ties)):
        assert at is None or float(want.grad[at].abs().max()) > 1e-3
        np.testing.assert_allclose(got.grad.numpy(), want.grad.numpy(), rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("weight_threshold", [None, 0.5])
def test_against_the_oracle(foam_factory, weight_threshold):
    """oracle.trace_forward(depth_quantiles=...) on the 64x48 frame against ray_quantiles over the oracle's own segments
    with density[cells] in float64: validity and cell agree, depths to rtol = 1e-6 (the oracle works in float32 with a
    running product, logf and a divide: a handful of float32 roundings).  Pairs whose validity or cell differ are left
    out of the depth comparison; they may be at most 0.5 % of all pairs.  Measured with seed 5: none differ, and the
    largest depth error is 1.4e-7 relative."""
    from oracle import oracle as O

    settings = {} if weight_threshold is None else {"weight_threshold": weight_threshold}
    fm, rays, starts, walk = S.image_case(foam_factory, **settings)
    rng = np.random.default_rng(5)
    q = -np.sort(-rng.uniform(0.02, 0.98, size=rays.shape[:-1] + (3,)).astype(np.float32), axis=-1)
    ref = O.trace_forward(fm["sh_degree"], fm["points"], fm["attributes"], fm["point_adjacency"],
                          fm["point_adjacency_offsets"], rays, starts, depth_quantiles=q, **settings)
    ref_depth = ref["depth"].reshape(-1, 3).astype(np.float64)
    ref_cells = ref["depth_indices"].reshape(-1, 3).astype(np.int64)
    ref_valid = ref_cells != 0xFFFFFFFF
    assert ((ref_depth == -1) == ~ref_valid).all()

    seg = {"offsets": torch.from_numpy(walk["offsets"]), "t_enter": torch.from_numpy(walk["t_enter"]),
           "t_exit": torch.from_numpy(walk["t_exit"])}
    cells = walk["cells"].astype(np.int64)
    sigma = torch.from_numpy(fm["attributes"][:, -1].astype(np.float64)[cells])
    assert float(sigma.min()) >= 0
    depth, entries = ray_quantiles(seg, sigma, torch.from_numpy(q.reshape(-1, 3)).double())
    depth, entries = depth.numpy(), entries.numpy()
    valid = entries >= 0
    got_cells = np.where(valid, cells[np.maximum(entries, 0)], 0xFFFFFFFF)
    same = (valid == ref_valid) & (got_cells == ref_cells)
    both = same & valid
    relative = np.abs(depth[both] - ref_depth[both]) / np.abs(ref_depth[both])
    print("weight_threshold %s: %d rays, %d entries, %d pairs, %d valid in the oracle; validity differs on %d, the cell "
          "on %d more; largest depth error %.3g relative, %.3g absolute, on depths of %.3g .. %.3g"
          % (weight_threshold, len(walk["offsets"]) - 1, len(cells), valid.size, ref_valid.sum(),
             (valid != ref_valid).sum(), (~same).sum() - (valid != ref_valid).sum(), relative.max(),
             np.abs(depth[both] - ref_depth[both]).max(), ref_depth[both].min(), ref_depth[both].max()))
    assert valid.size == 9216 and 0.2 < ref_valid.mean() < 0.8
    assert (~same).mean() <= 0.005
    assert (depth[~valid] == -1).all()
    np.testing.assert_allclose(depth[both], ref_depth[both], rtol=1e-6, atol=0.0)


def test_validation():
    seg = {"offsets": torch.tensor([0, 2, 3]), "t_exit": torch.tensor([1.0, 2.0, 0.5]),
           "t_enter": torch.tensor([0.0, 1.0, 0.0])}
    sigma, q = torch.rand(3), torch.tensor([[0.5, 0.2], [0.9, 0.1]])
    depth, entries = ray_quantiles(seg, sigma, q)
    assert depth.shape == (2, 2) and entries.shape == (2, 2)
    for backend in ("cuda", "HIP", ""):
        with pytest.raises(ValueError, match="backend must be None, 'hip' or 'torch'"):
            ray_quantiles(seg, sigma, q, backend=backend)
    bad = [
        ((seg, sigma.to(torch.float16), q.to(torch.float16)), "sigma must have float32 or float64 dtype"),
        ((seg, sigma.to(torch.int64), q), "sigma must have float32 or float64 dtype"),
        ((seg, sigma, q.double()), "quantiles must have the dtype and device of sigma"),
        ((seg, sigma.double(), q), "quantiles must have the dtype and device of sigma"),
        ((seg, sigma.reshape(3, 1), q), r"expected sigma \[S\] and quantiles \[R, Q\]"),
        ((seg, sigma, torch.tensor(0.5)), r"expected sigma \[S\] and quantiles \[R, Q\]"),
        ((seg, sigma, torch.zeros((2, 0))), r"expected sigma \[S\] and quantiles \[R, Q\]"),
        ((seg, sigma, q[:1]), "one row of Q per ray"),
        ((seg, sigma, torch.rand(3, 2)), "one row of Q per ray"),
        ((seg, sigma[:2], q), "one element per entry"),
        (({**seg, "t_enter": seg["t_enter"][:2]}, sigma, q), "one element per entry"),
        (({**seg, "t_exit": seg["t_exit"][:2]}, sigma, q), "one element per entry"),
        (({**seg, "offsets": seg["offsets"].to(torch.int32)}, sigma, q), r"seg\['offsets'\] must be int64"),
        (({**seg, "offsets": seg["offsets"].reshape(1, 3)}, sigma, q), r"seg\['offsets'\] must be int64"),
        (({**seg, "offsets": torch.tensor([0, 2, 2])}, sigma, q), r"seg\['offsets'\]\[-1\] must be the number"),
    ]
    for args, message in bad:
        with pytest.raises(RuntimeError, match=message):
            ray_quantiles(*args)
    with pytest.raises(RuntimeError, match="the kernel takes float32 CUDA sigma"):
        ray_quantiles(seg, sigma, q, backend="hip")
