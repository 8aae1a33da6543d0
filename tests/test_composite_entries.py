"""CPU: radfoam.composite_entries (torch backend and public surface) on segments of the CPU oracle -- the
300 rays tests/test_segments.py composites -- against a plain per-ray, per-entry loop in float64, against
composite_segments, and its gradients against finite differences and against autograd through composite_segments."""
import numpy as np
import pytest
import torch

import radfoam
import radfoam_amd
from radfoam import composite_entries, composite_segments
from tests.test_segments import _segments


def _loop(seg, sigma, values):
    """The definition, ray by ray, entry by entry, in float64."""
    off = seg["offsets"].numpy()
    t_enter, t_exit = seg["t_enter"].numpy(), seg["t_exit"].numpy()
    out = np.zeros((len(off) - 1, values.shape[1] + 1))
    for r in range(len(off) - 1):
        total = 0.0
        for e in range(off[r], off[r + 1]):
            dt = 0.0 if np.isinf(t_exit[e]) else max(float(t_exit[e]) - float(t_enter[e]), 0.0)
            x = sigma[e] * dt
            out[r, :-1] += np.exp(-total) * -np.expm1(-x) * values[e]
            total += x
        out[r, -1] = -np.expm1(-total)
    return out


def test_public_surface():
    assert "composite_entries" in radfoam_amd.__all__ and "composite_entries" in radfoam.__all__
    assert radfoam.composite_entries is radfoam_amd.segments.composite_entries


@pytest.mark.parametrize("channels", [1, 3, 7])
def test_matches_a_per_ray_loop(foam_factory, channels):
    """Random per-entry inputs at the foam's own scale: sigma is the density of the entry's cell times a random factor
    in 0.5 .. 1.5, values lie in 0 .. 1.  The scale matters to the bar, not to the operator: the restatement takes a
    ray's sums as differences of ONE cumulative sum over the whole list (composite_segments' way), so its exponents
    carry an absolute error of 2^-53 times that list-wide sum (about 100 here: 1e-14), and rtol = 1e-12 with no atol
    holds for rays of opacity down to 1e-2.  Values of both signs, whose sums cancel, are in the GPU test, where the bar
    has an absolute part."""
    fm, seg = _segments(foam_factory, 300)
    total = seg["cells"].numel()
    rng = np.random.default_rng(20 + channels)
    sigma = fm["attributes"][:, -1].astype(np.float64)[seg["cells"].numpy().astype(np.int64)]
    sigma = sigma * rng.uniform(0.5, 1.5, size=total)
    values = rng.uniform(0.0, 1.0, size=(total, channels))
    want = _loop(seg, sigma, values)
    assert want[:, -1].min() < 0.5 < want[:, -1].max() and want[:, :-1].max() > 0.1
    got = composite_entries(seg, torch.from_numpy(sigma), torch.from_numpy(values))
    assert got.dtype == torch.float64 and got.shape == (300, channels + 1)
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-12, atol=0.0)
    # float32 inputs: same values to float32 rounding of the result
    sigma32, values32 = sigma.astype(np.float32), values.astype(np.float32)
    got32 = composite_entries(seg, torch.from_numpy(sigma32), torch.from_numpy(values32), backend="torch")
    assert got32.dtype == torch.float32
    want32 = _loop(seg, sigma32.astype(np.float64), values32.astype(np.float64))
    np.testing.assert_allclose(got32.numpy(), want32, rtol=2e-7, atol=1e-7)


def test_per_cell_inputs_give_composite_segments(foam_factory):
    fm, seg = _segments(foam_factory, 300)
    rng = np.random.default_rng(5)
    density = torch.from_numpy(fm["attributes"][:, -1].astype(np.float64))
    rgb = torch.from_numpy(rng.uniform(0.0, 1.0, size=(density.numel(), 3)))
    cells = seg["cells"].to(torch.int64)
    got = composite_entries(seg, density[cells], rgb[cells])
    want = composite_segments(seg, density, rgb)
    assert float(want[:, 3].max()) > 0.5
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-12, atol=0.0)


def _small_case(foam_factory):
    """20 rays spread over the frame, C = 2; the list has entries with an infinite t_exit, and zero-length crossings
    (t_exit == t_enter, and t_exit < t_enter) are put on every 7th entry with a finite one."""
    _, seg = _segments(foam_factory, 20, stride=151)
    total = seg["cells"].numel()
    t_exit = seg["t_exit"].clone()
    flat = torch.arange(total)[torch.isfinite(t_exit)][::7]
    t_exit[flat] = seg["t_enter"][flat] - (torch.arange(flat.numel()) % 2).float() * 0.01
    seg = {**seg, "t_exit": t_exit}
    rng = np.random.default_rng(6)
    sigma = torch.from_numpy(rng.uniform(0.0, 5.0, size=total) * (rng.uniform(size=total) > 0.2))
    values = torch.from_numpy(rng.uniform(-1.0, 1.0, size=(total, 2)))
    assert bool(torch.isinf(seg["t_exit"]).any())
    assert bool((seg["t_exit"] == seg["t_enter"]).any()) and bool((seg["t_exit"] < seg["t_enter"]).any())
    assert bool((sigma == 0).any()) and bool((sigma > 1.0).any())
    return seg, sigma, values


def test_gradcheck(foam_factory):
    seg, sigma, values = _small_case(foam_factory)
    inputs = (sigma.clone().requires_grad_(True), values.clone().requires_grad_(True))
    assert torch.autograd.gradcheck(lambda s, v: composite_entries(seg, s, v), inputs, eps=1e-6, atol=1e-7, rtol=1e-5)


def test_time_gradients_are_those_of_composite_segments(foam_factory):
    """dL/dt_enter and dL/dt_exit are discontinuous at t_exit == t_enter (torch's clamp_min passes the gradient at
    equality), so finite differences say nothing there: they are held equal to autograd through composite_segments on
    a list in which every entry is a cell of its own, and to the closed form of DESIGN 4.11."""
    seg, sigma, values = _small_case(foam_factory)
    total = sigma.numel()
    rng = np.random.default_rng(7)
    weights = torch.from_numpy(rng.normal(size=(20, 4)))
    values = torch.cat([values, torch.from_numpy(rng.uniform(-1.0, 1.0, size=(total, 1)))], dim=1)
    t_exit64 = seg["t_exit"].double()
    assert bool((t_exit64 == seg["t_enter"].double()).any()) and bool((t_exit64 < seg["t_enter"].double()).any())

    def times():
        return seg["t_enter"].double().requires_grad_(True), t_exit64.clone().requires_grad_(True)

    t0, t1 = times()
    out = composite_entries({**seg, "t_enter": t0, "t_exit": t1}, sigma, values)
    (out * weights).sum().backward()
    own = {**seg, "cells": torch.arange(total, dtype=torch.int32).to(torch.uint32)}
    r0, r1 = times()
    ref = composite_segments({**own, "t_enter": r0, "t_exit": r1}, sigma, values)
    np.testing.assert_allclose(out.detach().numpy(), ref.detach().numpy(), rtol=1e-12, atol=0.0)
    (ref * weights).sum().backward()
    assert float(r1.grad.abs().max()) > 0.1
    np.testing.assert_allclose(t0.grad.numpy(), r0.grad.numpy(), rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(t1.grad.numpy(), r1.grad.numpy(), rtol=1e-12, atol=0.0)
    infinite = torch.isinf(t1.detach())
    assert bool((t1.grad[infinite] == 0).all()) and bool((t0.grad[infinite] == 0).all())
    np.testing.assert_array_equal(t0.grad.numpy(), -t1.grad.numpy())

    # the closed form, entry by entry
    off, g, v, s = seg["offsets"].numpy(), weights.numpy(), values.numpy(), sigma.numpy()
    a, b = seg["t_enter"].double().numpy(), t_exit64.numpy()
    dt = np.where(np.isinf(b), 0.0, np.maximum(b - a, 0.0))
    x = s * dt
    want = np.zeros(total)
    for r in range(20):
        e = np.arange(off[r], off[r + 1])
        through = np.exp(-(np.cumsum(x[e]) - x[e]))
        wq = through * (1.0 - np.exp(-x[e])) * (v[e] @ g[r, :3])
        later = wq.sum() - np.cumsum(wq)
        dx = through * np.exp(-x[e]) * (v[e] @ g[r, :3]) - later + g[r, 3] * np.exp(-x[e].sum())
        want[e] = np.where(np.isfinite(b[e]) & (b[e] >= a[e]), dx * s[e], 0.0)
    np.testing.assert_allclose(t1.grad.numpy(), want, rtol=1e-9, atol=1e-12)


def test_empty_batch_and_rays_without_entries():
    none = {"offsets": torch.zeros(1, dtype=torch.int64), "cells": torch.zeros(0, dtype=torch.uint32),
            "t_exit": torch.zeros(0), "t_enter": torch.zeros(0)}
    out = composite_entries(none, torch.zeros(0, dtype=torch.float64), torch.zeros((0, 5), dtype=torch.float64))
    assert out.shape == (0, 6) and out.dtype == torch.float64
    # six rays; the first, two in the middle and the last without entries
    seg = {"offsets": torch.tensor([0, 0, 2, 2, 2, 3, 3]), "t_exit": torch.tensor([1.0, float("inf"), 0.5]),
           "t_enter": torch.tensor([0.0, 1.0, 0.0])}
    sigma = torch.tensor([0.7, 2.0, 3.0], dtype=torch.float64, requires_grad=True)
    values = torch.tensor([[0.5, -1.0], [1.0, 1.0], [-0.25, 0.75]], dtype=torch.float64, requires_grad=True)
    out = composite_entries(seg, sigma, values)
    got = out.detach().numpy()
    np.testing.assert_allclose(got, _loop(seg, sigma.detach().numpy(), values.detach().numpy()), rtol=1e-12)
    assert (got[[0, 2, 3, 5]] == 0).all() and (got[[1, 4]] != 0).all()
    out.sum().backward()
    assert float(sigma.grad[1]) == 0 and bool((values.grad[1] == 0).all())     # behind an infinite t_exit: dt = 0
    # rays, none of which has an entry (float32)
    only_empty = {"offsets": torch.zeros(4, dtype=torch.int64), "t_exit": torch.zeros(0), "t_enter": torch.zeros(0)}
    out = composite_entries(only_empty, torch.zeros(0), torch.zeros((0, 1)))
    assert out.shape == (3, 2) and out.dtype == torch.float32 and bool((out == 0).all())


def test_validation():
    seg = {"offsets": torch.tensor([0, 2, 3]), "t_exit": torch.tensor([1.0, 2.0, 0.5]),
           "t_enter": torch.tensor([0.0, 1.0, 0.0])}
    sigma, values = torch.rand(3), torch.rand(3, 2)
    assert composite_entries(seg, sigma, values).shape == (2, 3)
    with pytest.raises(ValueError, match="backend must be None, 'hip' or 'torch'"):
        composite_entries(seg, sigma, values, backend="cuda")
    bad = [
        ((seg, sigma.to(torch.float16), values.to(torch.float16)), "sigma must have float32 or float64 dtype"),
        ((seg, sigma, values.double()), "values must have the dtype and device of sigma"),
        ((seg, sigma.reshape(3, 1), values), r"expected sigma \[S\] and values \[S, C\]"),
        ((seg, sigma, values.reshape(3, 2, 1)), r"expected sigma \[S\] and values \[S, C\]"),
        ((seg, sigma, values[:, 0]), r"expected sigma \[S\] and values \[S, C\]"),
        ((seg, sigma, values[:, :0]), r"expected sigma \[S\] and values \[S, C\]"),
        ((seg, sigma, values[:2]), "one element .* per entry"),
        ((seg, sigma[:2], values[:2]), "one element .* per entry"),
        (({**seg, "t_enter": seg["t_enter"][:2]}, sigma, values), "one element .* per entry"),
        (({**seg, "offsets": seg["offsets"].to(torch.int32)}, sigma, values), r"seg\['offsets'\] must be int64"),
        (({**seg, "offsets": torch.tensor([0, 2, 2])}, sigma, values), r"seg\['offsets'\]\[-1\] must be the number"),
    ]
    for args, message in bad:
        with pytest.raises(RuntimeError, match=message):
            composite_entries(*args)
    with pytest.raises(RuntimeError, match="the kernel takes float32 CUDA sigma"):
        composite_entries(seg, sigma, values, backend="hip")
