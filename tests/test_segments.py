"""CPU: radfoam.composite_segments on segments of the CPU oracle (oracle.trace_paths) -- 300 rays of the 64x48 frame of
foam_factory(3000, 2, 21) -- against a plain per-ray loop in float64, and its gradients against finite differences."""
import numpy as np
import torch

from radfoam import composite_segments
from tests import segments_ref as S


def _segments(foam_factory, num_rays, stride=1):
    """`num_rays` rays of the image case, every `stride`-th in row-major order: (fm, dict of torch tensors as
    trace_segments returns them)."""
    fm, _, _, ref = S.image_case(foam_factory)
    rays = np.arange(num_rays) * stride
    counts = ref["counts"][rays]
    entries = np.concatenate([np.arange(ref["offsets"][r], ref["offsets"][r + 1]) for r in rays])
    seg = {"offsets": torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)),
           "cells": torch.from_numpy(ref["cells"][entries]),
           "t_exit": torch.from_numpy(ref["t_exit"][entries]),
           "t_enter": torch.from_numpy(ref["t_enter"][entries])}
    assert seg["cells"].dtype == torch.uint32 and seg["t_exit"].dtype == torch.float32
    return fm, seg


def _loop(seg, density, rgb):
    """The definition, ray by ray, entry by entry, in float64."""
    off = seg["offsets"].numpy()
    cells, t_enter, t_exit = (seg[k].numpy() for k in ("cells", "t_enter", "t_exit"))
    out = np.zeros((len(off) - 1, 4))
    for r in range(len(off) - 1):
        T = 1.0
        for e in range(off[r], off[r + 1]):
            dt = 0.0 if np.isinf(t_exit[e]) else max(float(t_exit[e]) - float(t_enter[e]), 0.0)
            alpha = 1.0 - np.exp(-density[cells[e]] * dt)
            out[r, :3] += T * alpha * rgb[cells[e]]
            T *= 1.0 - alpha
        out[r, 3] = 1.0 - T
    return out


def test_composite_matches_a_per_ray_loop(foam_factory):
    fm, seg = _segments(foam_factory, 300)
    rng = np.random.default_rng(5)
    density = fm["attributes"][:, -1].astype(np.float64)
    rgb = rng.uniform(0.0, 1.0, size=(len(density), 3))
    want = _loop(seg, density, rgb)
    assert want[:, 3].min() < 0.5 < want[:, 3].max()          # the rays see both empty space and opaque cells
    got = composite_segments(seg, torch.from_numpy(density), torch.from_numpy(rgb))
    assert got.dtype == torch.float64 and got.shape == (300, 4)
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-12, atol=0.0)
    # float32 inputs: same values to float32 rounding of the result
    got32 = composite_segments(seg, torch.from_numpy(density.astype(np.float32)), torch.from_numpy(rgb.astype(np.float32)))
    assert got32.dtype == torch.float32
    want32 = _loop(seg, density.astype(np.float32).astype(np.float64), rgb.astype(np.float32).astype(np.float64))
    np.testing.assert_allclose(got32.numpy(), want32, rtol=2e-7, atol=1e-7)


def test_empty_rays_and_empty_batch():
    density, rgb = torch.rand(5, dtype=torch.float64), torch.rand(5, 3, dtype=torch.float64)
    none = {"offsets": torch.zeros(1, dtype=torch.int64), "cells": torch.zeros(0, dtype=torch.uint32),
            "t_exit": torch.zeros(0), "t_enter": torch.zeros(0)}
    assert composite_segments(none, density, rgb).shape == (0, 4)
    # three rays, the middle one without entries
    seg = {"offsets": torch.tensor([0, 2, 2, 3]), "cells": torch.tensor([1, 2, 4], dtype=torch.int32).to(torch.uint32),
           "t_exit": torch.tensor([1.0, float("inf"), 0.5]), "t_enter": torch.tensor([0.0, 1.0, 0.0])}
    got = composite_segments(seg, density, rgb).numpy()
    np.testing.assert_allclose(got, _loop(seg, density.numpy(), rgb.numpy()), rtol=1e-12)
    assert (got[1] == 0).all()


def test_gradcheck(foam_factory):
    """20 rays spread over the frame.  Element by element (no fast mode) over the density and colour of every cell they
    cross; the other cells have no gradient and are left out of the perturbed inputs, not of the call."""
    fm, seg = _segments(foam_factory, 20, stride=151)
    rng = np.random.default_rng(6)
    density = torch.from_numpy(fm["attributes"][:, -1].astype(np.float64))
    rgb = torch.from_numpy(rng.uniform(0.0, 1.0, size=(density.numel(), 3)))
    touched = torch.unique(seg["cells"].to(torch.int64))
    assert 100 < touched.numel() < density.numel()
    assert (density[touched] > 1.0).any() and (density[touched] == 0).any()

    def composite(d_part, c_part):
        return composite_segments(seg, density.index_put((touched,), d_part), rgb.index_put((touched,), c_part))

    inputs = (density[touched].clone().requires_grad_(True), rgb[touched].clone().requires_grad_(True))
    assert torch.autograd.gradcheck(composite, inputs, eps=1e-6, atol=1e-7, rtol=1e-5)
    # cells no ray crosses get a zero gradient, not none
    d, c = density.clone().requires_grad_(True), rgb.clone().requires_grad_(True)
    composite_segments(seg, d, c).sum().backward()
    untouched = torch.ones(density.numel(), dtype=torch.bool)
    untouched[touched] = False
    assert (d.grad[untouched] == 0).all() and (c.grad[untouched] == 0).all() and (c.grad[touched] != 0).any()
