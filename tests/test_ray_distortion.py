"""CPU: radfoam.ray_distortion (torch backend and public surface) on hand-built lists: against the literal
|m_i - m_j| double sum in a per-ray float64 loop, its gradients against finite differences, against the closed form of
DESIGN 4.13 evaluated in a float64 loop and, on exact ties, against autograd through a clamp_min restatement; Euler's
identity for a form of degree 2 in the weights; validation; the build lists."""
import os

import numpy as np
import pytest
import torch

import radfoam
import radfoam_amd
from radfoam import ray_distortion

COUNTS = [0, 1, 5, 0, 0, 70, 33, 2, 7, 0]          # empty rays first, in the middle and last; at most 70 entries


def _list(counts, seed, ties=True):
    """A list with the given entries per ray, float64: per ray an increasing sequence of crossings that starts at
    0 .. 0.5 with steps of 0.05 .. 0.3; inverted entries (t_exit < t_enter) sprinkled in and, with `ties`, zero-length
    ones (t_exit == t_enter); +inf on the last entry of every odd ray and of the longest; sigma in 0.2 .. 4 with exact
    zeros, scaled by 8 / n on a ray of n > 8 entries so that the sum of x over a ray stays near 2.5 and late entries keep
    weight.  The midpoints of the entries that carry weight do not decrease along a ray."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, dtype=np.int64)
    total = int(counts.sum())
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    t_enter, t_exit, sigma = np.zeros(total), np.zeros(total), np.zeros(total)
    for r, n in enumerate(counts):
        if n == 0:
            continue
        e = slice(offsets[r], offsets[r] + n)
        edges = rng.uniform(0.0, 0.5) + np.concatenate([[0.0], np.cumsum(rng.uniform(0.05, 0.3, size=n))])
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


def _contracted(seg):
    """s = t / (1 + t) of both times.  An infinite t_exit gives nan, on purpose: the entry has no weight, and nothing of
    it may reach the result or a gradient."""
    return tuple(t / (1 + t) for t in (seg["t_enter"].detach().clone(), seg["t_exit"].detach().clone()))


def _weights(t_enter, t_exit, sigma):
    """w of one ray, entry by entry."""
    w, total = np.zeros(len(sigma)), 0.0
    for i in range(len(sigma)):
        dt = 0.0 if np.isinf(t_exit[i]) else max(t_exit[i] - t_enter[i], 0.0)
        w[i] = np.exp(-total) * -np.expm1(-sigma[i] * dt)
        total += sigma[i] * dt
    return w


def _measure(t_enter, t_exit, a, b):
    """m, d of one ray: zeros, selected, where t_exit is infinite."""
    m = np.array([0.0 if np.isinf(t1) else (x + y) / 2 for t1, x, y in zip(t_exit, a, b)])
    d = np.array([0.0 if np.isinf(t1) else max(y - x, 0.0) for t1, x, y in zip(t_exit, a, b)])
    return m, d


def _double_sum(seg, sigma, s=None):
    """Mip-NeRF 360's sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 d_i, literally, ray by ray."""
    off, t_enter, t_exit, sigma = seg["offsets"].numpy(), seg["t_enter"].numpy(), seg["t_exit"].numpy(), sigma.numpy()
    a, b = (t_enter, t_exit) if s is None else (s[0].numpy(), s[1].numpy())
    out = np.zeros(len(off) - 1)
    for r in range(len(off) - 1):
        e = slice(off[r], off[r + 1])
        w = _weights(t_enter[e], t_exit[e], sigma[e])
        m, d = _measure(t_enter[e], t_exit[e], a[e], b[e])
        carrying = m[w > 0]
        assert (np.diff(carrying) >= 0).all(), "the list must have non-decreasing midpoints where there is weight"
        for i in range(len(w)):
            for j in range(len(w)):
                out[r] += w[i] * w[j] * abs(m[i] - m[j])
            out[r] += w[i] * w[i] * d[i] / 3
    return out


def _closed_form(seg, sigma, grad_out, s=None):
    """DESIGN 4.13's formulas in a float64 loop: (out, grad_sigma, grad_t_enter, grad_t_exit, grad_a, grad_b, sum w g);
    the gradient of the times is the part through w alone."""
    off, t_enter, t_exit, sigma = seg["offsets"].numpy(), seg["t_enter"].numpy(), seg["t_exit"].numpy(), sigma.numpy()
    a, b = (t_enter, t_exit) if s is None else (s[0].numpy(), s[1].numpy())
    num_rays, total = len(off) - 1, len(sigma)
    out, euler = np.zeros(num_rays), np.zeros(num_rays)
    g_sigma, g_enter, g_exit, g_a, g_b = (np.zeros(total) for _ in range(5))
    for r in range(num_rays):
        lo, n = off[r], off[r + 1] - off[r]
        e = slice(lo, lo + n)
        w = _weights(t_enter[e], t_exit[e], sigma[e])
        m, d = _measure(t_enter[e], t_exit[e], a[e], b[e])
        for i in range(n):
            k = lo + i
            infinite = np.isinf(t_exit[k])
            dt = 0.0 if infinite else max(t_exit[k] - t_enter[k], 0.0)
            w_lt, m_lt = w[:i].sum(), (w[:i] * m[:i]).sum()
            w_gt, m_gt = w[i + 1:].sum(), (w[i + 1:] * m[i + 1:]).sum()
            out[r] += 2 * w[i] * (m[i] * w_lt - m_lt) + w[i] * w[i] * d[i] / 3

            def dout_dw(j):
                return (2 * (m[j] * w[:j].sum() - (w[:j] * m[:j]).sum())
                        + 2 * ((w[j + 1:] * m[j + 1:]).sum() - m[j] * w[j + 1:].sum()) + 2 * w[j] * d[j] / 3)

            g = dout_dw(i)
            euler[r] += w[i] * g
            dout_dm, dout_dd = 2 * w[i] * (w_lt - w_gt), w[i] * w[i] / 3
            if not infinite:
                widens = 1.0 if b[k] >= a[k] else 0.0
                g_b[k] = grad_out[r] * (dout_dm / 2 + widens * dout_dd)
                g_a[k] = grad_out[r] * (dout_dm / 2 - widens * dout_dd)
            through = np.exp(-sum(
                sigma[j] * (0.0 if np.isinf(t_exit[j]) else max(t_exit[j] - t_enter[j], 0.0)) for j in range(lo, k)))
            later = sum(w[j] * dout_dw(j) for j in range(i + 1, n))
            dx = grad_out[r] * (through * np.exp(-sigma[k] * dt) * g - later)
            g_sigma[k] = dx * dt
            if not infinite and t_exit[k] >= t_enter[k]:
                g_exit[k] = dx * sigma[k]
                g_enter[k] = -g_exit[k]
    return out, g_sigma, g_enter, g_exit, g_a, g_b, euler


def _leaves(seg, sigma, s=None):
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    t0, t1, sig = leaf(seg["t_enter"]), leaf(seg["t_exit"]), leaf(sigma)
    s = None if s is None else (leaf(s[0]), leaf(s[1]))
    return {**seg, "t_enter": t0, "t_exit": t1}, sig, s


def _call(seg, sigma, s, **kw):
    return ray_distortion(seg, sigma, **kw) if s is None else ray_distortion(seg, sigma, s[0], s[1], **kw)


def test_public_surface():
    assert "ray_distortion" in radfoam_amd.__all__ and "ray_distortion" in radfoam.__all__
    assert radfoam.ray_distortion is radfoam_amd.segments.ray_distortion


def test_sources_are_built_but_not_part_of_the_source_hash():
    from radfoam_amd import _lib, build

    names = lambda paths: {os.path.basename(p) for p in paths}
    assert "rf_distortion.hip" in names(build.EXTRA_SOURCES)
    assert {"radfoam_hip_distortion.h", "rf_ray_sweep.hpp", "rf_segments_face.hpp"} <= names(build.EXTRA_HEADERS)
    assert not names(build.SOURCES + build.HEADERS) & {"rf_distortion.hip", "radfoam_hip_distortion.h"}
    assert not names(build.SOURCES + build.HEADERS) & names(build.EXTRA_SOURCES + build.EXTRA_HEADERS)
    lib = _lib.load()
    for name in ("rf_ray_distortion_forward", "rf_ray_distortion_backward", "rf_distortion_rays_per_wave"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert 1 <= lib.rf_distortion_rays_per_wave() <= 63
    none = [None] * 5
    assert lib.rf_ray_distortion_forward(0, None, 0, *none, None, None) == 0                   # nothing to do
    assert lib.rf_ray_distortion_backward(0, None, 0, *none, None, *none, None) == 0
    dummy = np.zeros(64).ctypes.data
    assert lib.rf_ray_distortion_forward(5, None, 3, *none, dummy, None) == -1
    assert "null pointer" in _lib.last_error()
    assert lib.rf_ray_distortion_forward(5, dummy, 3, dummy, dummy, dummy, dummy, None, dummy, None) == -1
    assert "both given or both null" in _lib.last_error()
    assert lib.rf_ray_distortion_backward(5, None, 3, *none, None, dummy, None, None, None, None, None) == -1
    assert "null pointer" in _lib.last_error()
    assert lib.rf_ray_distortion_backward(5, dummy, 3, dummy, dummy, dummy, None, None, dummy, dummy, None, None,
                                          dummy, None, None) == -1
    assert "without s_enter" in _lib.last_error()


@pytest.mark.parametrize("contracted", [False, True])
def test_matches_the_double_sum(contracted):
    """rtol = 1e-12 with no atol.  The restatement takes W< and M< as differences of list-wide cumulative sums, so each
    carries an absolute error of about 2^-53 times the list-wide sum (at most 6 for w, one per ray with entries, and
    about 30 for w m, m up to 12): 1e-15 to 1e-14 against distortions of 1e-3 and more on every ray that has weight."""
    seg, sigma = _list(COUNTS, seed=1)
    assert bool(torch.isinf(seg["t_exit"]).any()) and bool((seg["t_exit"] == seg["t_enter"]).any())
    assert bool((seg["t_exit"] < seg["t_enter"]).any()) and bool((sigma == 0).any())
    s = _contracted(seg) if contracted else None
    assert s is None or bool(torch.isnan(s[1]).any())
    want = _double_sum(seg, sigma, s)
    got = _call(seg, sigma, s)
    assert got.dtype == torch.float64 and got.shape == (len(COUNTS),)
    counts = np.asarray(COUNTS)
    assert (got.numpy()[counts == 0] == 0).all()
    weighted = want[want > 0]            # a ray of nothing but weightless entries gives an exact 0 on both sides
    assert len(weighted) >= 4 and weighted.min() > (1e-4 if contracted else 1e-3)
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-12, atol=0.0)
    # float32 inputs: the same to a float32 rounding of the result
    seg32 = {**seg, "t_enter": seg["t_enter"].float(), "t_exit": seg["t_exit"].float()}
    s32 = None if s is None else (s[0].float(), s[1].float())
    got32 = _call(seg32, sigma.float(), s32, backend="torch")
    assert got32.dtype == torch.float32
    seg64 = {**seg, "t_enter": seg32["t_enter"].double(), "t_exit": seg32["t_exit"].double()}
    want32 = _call(seg64, sigma.float().double(), None if s is None else (s32[0].double(), s32[1].double()))
    np.testing.assert_allclose(got32.numpy(), want32.numpy(), rtol=2e-7, atol=1e-7)


def test_empty_batch_and_rays_without_entries():
    none = {"offsets": torch.zeros(1, dtype=torch.int64), "t_exit": torch.zeros(0), "t_enter": torch.zeros(0)}
    out = ray_distortion(none, torch.zeros(0, dtype=torch.float64))
    assert out.shape == (0,) and out.dtype == torch.float64
    only_empty = {"offsets": torch.zeros(4, dtype=torch.int64), "t_exit": torch.zeros(0), "t_enter": torch.zeros(0)}
    out = ray_distortion(only_empty, torch.zeros(0), torch.zeros(0), torch.zeros(0))
    assert out.shape == (3,) and out.dtype == torch.float32 and bool((out == 0).all())
    # one entry behind an infinite t_exit alone: no weight, no distortion, zero gradients
    seg = {"offsets": torch.tensor([0, 1]), "t_enter": torch.tensor([0.5], dtype=torch.float64, requires_grad=True),
           "t_exit": torch.tensor([float("inf")], dtype=torch.float64, requires_grad=True)}
    sigma = torch.tensor([2.0], dtype=torch.float64, requires_grad=True)
    out = ray_distortion(seg, sigma)
    out.sum().backward()
    assert float(out.detach()) == 0 and float(sigma.grad) == 0 and float(seg["t_enter"].grad) == 0 and float(seg["t_exit"].grad) == 0


def _gradcheck_case():
    counts = [3, 0, 7, 5, 1, 9, 4, 6, 0, 2, 8, 5, 3, 7, 1, 6, 4, 12, 5, 3]
    seg, sigma = _list(counts, seed=2, ties=False)
    assert len(counts) == 20 and not bool((seg["t_exit"] == seg["t_enter"]).any())
    assert bool(torch.isinf(seg["t_exit"]).any()) and bool((seg["t_exit"] < seg["t_enter"]).any())
    return seg, sigma


@pytest.mark.parametrize("contracted", [False, True])
def test_gradcheck(contracted):
    seg, sigma = _gradcheck_case()
    infinite = torch.isinf(seg["t_exit"])
    if contracted:
        s = _contracted(seg)
        assert not bool((s[1] == s[0]).any()) and bool(torch.isnan(s[1][infinite]).all())
        fn = lambda sig, t0, t1, s0, s1: ray_distortion({**seg, "t_enter": t0, "t_exit": t1}, sig, s0, s1)
        inputs = (sigma, seg["t_enter"], seg["t_exit"]) + s
    else:
        fn = lambda sig, t0, t1: ray_distortion({**seg, "t_enter": t0, "t_exit": t1}, sig)
        inputs = (sigma, seg["t_enter"], seg["t_exit"])
    inputs = tuple(t.clone().requires_grad_(True) for t in inputs)
    assert torch.autograd.gradcheck(fn, inputs, eps=1e-6, atol=1e-7, rtol=1e-5)
    fn(*inputs).sum().backward()
    for t in inputs:                                       # behind an infinite t_exit: exact zeros, selected
        assert bool((t.grad[infinite] == 0).all()) and float(t.grad.abs().max()) > 1e-3


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("contracted", [False, True])
def test_closed_form_and_euler_identity(contracted, ties):
    """DESIGN 4.13's gradient formulas, with every sum over a ray's earlier or later entries written out, equal autograd
    to 1e-10; and sum_i w_i (d out / d w_i) = 2 out[r], which is what lets the kernel do without a third sweep.  With
    `ties`, the list has t_exit == t_enter (and with them s_exit == s_enter) exactly: [b >= a] is clamp_min's."""
    seg, sigma = _list(COUNTS, seed=3, ties=ties) if ties else _gradcheck_case()
    assert bool((seg["t_exit"] == seg["t_enter"]).any()) == ties
    s = _contracted(seg) if contracted else None
    assert s is None or bool((s[1] == s[0]).any()) == ties
    num_rays = seg["offsets"].numel() - 1
    grad_out = np.random.default_rng(4).normal(size=num_rays)
    seg_l, sigma_l, s_l = _leaves(seg, sigma, s)
    out = _call(seg_l, sigma_l, s_l)
    out.backward(torch.from_numpy(grad_out))
    want_out, g_sigma, g_enter, g_exit, g_a, g_b, euler = _closed_form(seg, sigma, grad_out, s)
    close = lambda got, want: np.testing.assert_allclose(got.detach().numpy(), want, rtol=1e-10, atol=1e-10)
    close(out, want_out)
    close(sigma_l.grad, g_sigma)
    assert float(sigma_l.grad.abs().max()) > 1e-2 and np.abs(g_b).max() > 1e-2
    if contracted:
        close(seg_l["t_enter"].grad, g_enter)
        close(seg_l["t_exit"].grad, g_exit)
        close(s_l[0].grad, g_a)
        close(s_l[1].grad, g_b)
    else:
        close(seg_l["t_enter"].grad, g_enter + g_a)
        close(seg_l["t_exit"].grad, g_exit + g_b)
    np.testing.assert_allclose(euler, 2 * out.detach().numpy(), rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("contracted", [False, True])
def test_tie_convention_is_clamp_min(contracted):
    """On a list with exact ties the gradients equal autograd through a restatement, ray by ray with torch operations,
    in which both max(., 0) are clamp_min.  An entry with t_exit == t_enter has no weight, so its tie shows in the
    gradient of the times through w alone; the tie in d shows where s_exit == s_enter on an entry that has weight (a
    measure that stands still over the entry: the midpoints still do not decrease)."""
    seg, sigma = _list(COUNTS, seed=5)
    ties = seg["t_exit"] == seg["t_enter"]
    assert int(ties.sum()) >= 5
    s = s_ties = None
    if contracted:
        s = _contracted(seg)
        s_ties = torch.zeros_like(ties)
        s_ties[torch.arange(ties.numel())[torch.isfinite(seg["t_exit"]) & (seg["t_exit"] > seg["t_enter"])][::4]] = True
        s[1][s_ties] = s[0][s_ties]
        assert int(s_ties.sum()) >= 10
    grad_out = torch.from_numpy(np.random.default_rng(6).normal(size=len(COUNTS)))
    seg_l, sigma_l, s_l = _leaves(seg, sigma, s)
    _call(seg_l, sigma_l, s_l).backward(grad_out)

    seg_r, sigma_r, s_r = _leaves(seg, sigma, s)
    off, rows = seg["offsets"].tolist(), []
    for r in range(len(COUNTS)):
        e = slice(off[r], off[r + 1])
        t0, t1 = seg_r["t_enter"][e], seg_r["t_exit"][e]
        finite = torch.isfinite(t1.detach())
        t0, t1, sig = t0[finite], t1[finite], sigma_r[e][finite]           # an infinite t_exit: no weight, last entry
        a, b = (t0, t1) if s is None else (s_r[0][e][finite], s_r[1][e][finite])
        x = sig * (t1 - t0).clamp_min(0.0)
        w = torch.exp(-(torch.cumsum(x, 0) - x)) * (1 - torch.exp(-x))
        m, d = (a + b) / 2, (b - a).clamp_min(0.0)
        rows.append((2 * w * (m * (torch.cumsum(w, 0) - w) - (torch.cumsum(w * m, 0) - w * m)) + w * w * d / 3).sum())
    torch.stack(rows).backward(grad_out)
    pairs = [(sigma_l, sigma_r, None), (seg_l["t_enter"], seg_r["t_enter"], ties), (seg_l["t_exit"], seg_r["t_exit"], ties)]
    pairs += [] if s is None else [(s_l[0], s_r[0], s_ties), (s_l[1], s_r[1], s_ties)]
    for got, want, at in pairs:
        assert at is None or float(want.grad[at].abs().max()) > 1e-3
        np.testing.assert_allclose(got.grad.numpy(), want.grad.numpy(), rtol=1e-10, atol=1e-12)
    if contracted:                       # d's half of the gradient is there: it is what keeps grad_b from being grad_a
        assert float((s_r[1].grad - s_r[0].grad)[s_ties].abs().max()) > 1e-3


def test_validation():
    seg = {"offsets": torch.tensor([0, 2, 3]), "t_exit": torch.tensor([1.0, 2.0, 0.5]),
           "t_enter": torch.tensor([0.0, 1.0, 0.0])}
    sigma, s0, s1 = torch.rand(3), torch.tensor([0.0, 0.5, 0.0]), torch.tensor([0.5, 0.7, 0.3])
    assert ray_distortion(seg, sigma).shape == (2,) and ray_distortion(seg, sigma, s0, s1).shape == (2,)
    for backend in ("cuda", "HIP", ""):
        with pytest.raises(ValueError, match="backend must be None, 'hip' or 'torch'"):
            ray_distortion(seg, sigma, backend=backend)
    bad = [
        ((seg, sigma.to(torch.float16)), "sigma must have float32 or float64 dtype"),
        ((seg, sigma.to(torch.int64)), "sigma must have float32 or float64 dtype"),
        ((seg, sigma, s0), "both be given or both be omitted"),
        ((seg, sigma, None, s1), "both be given or both be omitted"),
        ((seg, sigma, s0.double(), s1.double()), "must have the dtype and device of sigma"),
        ((seg, sigma, s0, s1.double()), "must have the dtype and device of sigma"),
        ((seg, sigma.reshape(3, 1)), r"expected sigma \[S\]"),
        ((seg, sigma, s0.reshape(3, 1), s1), r"expected sigma \[S\]"),
        ((seg, sigma[:2]), "one element per entry"),
        ((seg, sigma, s0[:2], s1), "one element per entry"),
        ((seg, sigma, s0, s1[:2]), "one element per entry"),
        (({**seg, "t_enter": seg["t_enter"][:2]}, sigma), "one element per entry"),
        (({**seg, "t_exit": seg["t_exit"][:2]}, sigma), "one element per entry"),
        (({**seg, "offsets": seg["offsets"].to(torch.int32)}, sigma), r"seg\['offsets'\] must be int64"),
        (({**seg, "offsets": seg["offsets"].reshape(1, 3)}, sigma), r"seg\['offsets'\] must be int64"),
        (({**seg, "offsets": torch.tensor([0, 2, 2])}, sigma), r"seg\['offsets'\]\[-1\] must be the number"),
    ]
    for args, message in bad:
        with pytest.raises(RuntimeError, match=message):
            ray_distortion(*args)
    with pytest.raises(RuntimeError, match="the kernel takes float32 CUDA sigma"):
        ray_distortion(seg, sigma, backend="hip")
