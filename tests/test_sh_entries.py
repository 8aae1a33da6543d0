"""CPU: radfoam.sh_entries: the public surface, the build lists and the C-ABI's argument checks; the torch
backend against an entry-by-entry float64 loop and under gradcheck; the chain gather_cells -> sh_entries ->
composite_entries against the oracle's trace_forward at degrees 1 .. 3 and against its trace_backward at degree 2; and
the example at toy size."""
import os
import sys

import numpy as np
import pytest
import torch

import radfoam
import radfoam_amd
from radfoam import cell_entries, composite_entries, gather_cells, sh_entries
from tests import helpers as H
from tests import segments_ref as S

# six rays of 0, 3, 0, 4, 1 and 0 entries: empty rays first, in the middle and last
OFFSETS = torch.tensor([0, 0, 3, 3, 7, 8, 8], dtype=torch.int64)
NUM_CELLS = 5                                                      # cell 4 has no entry


def _basis(d, degree):
    """Y_0 .. Y_{K-1} at one unit vector, float64: the polynomials of the oracle's sh_basis, written out once more."""
    x, y, z = (float(v) for v in d)
    sh = [0.28209479177387814]
    if degree > 0:
        sh += [-0.4886025119029199 * y, 0.4886025119029199 * z, -0.4886025119029199 * x]
    if degree > 1:
        sh += [1.0925484305920792 * x * y, -1.0925484305920792 * y * z,
               0.31539156525252005 * (2 * z * z - x * x - y * y), -1.0925484305920792 * x * z, 0.5462742152960396 * (x * x - y * y)]
    if degree > 2:
        sh += [-0.5900435899266435 * y * (3 * x * x - y * y), 2.890611442640554 * x * y * z,
               -0.4570457994644658 * y * (4 * z * z - x * x - y * y),
               0.3731763325901154 * z * (2 * z * z - 3 * x * x - 3 * y * y),
               -0.4570457994644658 * x * (4 * z * z - x * x - y * y), 1.445305721320277 * z * (x * x - y * y),
               -0.5900435899266435 * x * (x * x - 3 * y * y)]
    return np.array(sh)


def _loop(offsets, cells, coeffs, directions, degree):
    """(rgb, pre) [S, 3]: entry by entry in float64."""
    off, coeffs = offsets.tolist(), coeffs.detach().double().numpy()
    dirs = directions.detach().double().reshape(-1, 3).numpy()
    pre = np.zeros((off[-1], 3))
    for r in range(len(off) - 1):
        y = _basis(dirs[r] / np.sqrt((dirs[r] ** 2).sum()), degree)
        for e in range(off[r], off[r + 1]):
            for c in range(3):
                pre[e, c] = 0.5 + sum(y[k] * coeffs[cells[e], 3 * k + c] for k in range(len(y)))
    return np.maximum(pre, 0.0), pre


def _small_case(degree, seed):
    """(seg, index, cells, coeffs, directions): coefficients whose colours stay 0.1 clear of the clamp, and cells 1 and
    3 pushed well below it through their constant term."""
    rng = np.random.default_rng(seed)
    cells = [0, 1, 2, 3, 3, 1, 0, 2]
    seg = {"offsets": OFFSETS, "cells": torch.tensor(cells, dtype=torch.int64)}
    width = 3 * (degree + 1) ** 2
    coeffs = rng.uniform(-1.0, 1.0, size=(NUM_CELLS, width)) * (0.4 / (0.75 * (width // 3)))   # |sum| <= 0.4
    coeffs[1, :3] -= 5.0                                           # 0.5 - 5 C0 = -0.91
    coeffs[3, 1] -= 5.0
    directions = rng.normal(size=(6, 3)) * rng.uniform(0.5, 3.0, size=(6, 1))                 # not unit length
    return seg, cell_entries(seg, NUM_CELLS), cells, torch.from_numpy(coeffs), torch.from_numpy(directions)


def test_public_surface_build_lists_and_argument_checks():
    from radfoam_amd import _lib, build

    assert "sh_entries" in radfoam_amd.__all__ and "sh_entries" in radfoam.__all__
    assert radfoam.sh_entries is radfoam_amd.sh_entries is sys.modules["radfoam_amd.sh_entries"].sh_entries
    names = lambda paths: {os.path.basename(p) for p in paths}
    assert "rf_sh_entries.hip" in names(build.EXTRA_SOURCES)
    assert {"radfoam_hip_sh_entries.h", "rf_cell_sweep.hpp"} <= names(build.EXTRA_HEADERS)
    assert "rf_cell_sweep.hpp" not in names(build.SOURCES + build.HEADERS)
    assert not names(build.SOURCES + build.HEADERS) & names(build.EXTRA_SOURCES + build.EXTRA_HEADERS)
    assert "rf_math.hpp" in names(build.HEADERS)                   # included, and still part of the source hash
    for path in build.EXTRA_SOURCES + build.EXTRA_HEADERS:
        assert os.path.exists(path), path
    lib = _lib.load()
    symbols = ("rf_sh_entries_group", "rf_sh_entries_forward", "rf_sh_entries_workspace_bytes",
               "rf_sh_entries_backward_coeffs", "rf_sh_entries_backward_directions")
    for name in symbols:
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.rf_sh_entries_group() in (1, 2, 4, 8)
    chunk = lib.rf_reduce_entries_chunk()
    # two rows of 3 K doubles per chunk
    assert lib.rf_sh_entries_workspace_bytes(0, 3) == 0 and lib.rf_sh_entries_workspace_bytes(-5, 3) == 0
    assert lib.rf_sh_entries_workspace_bytes(5, 4) == 0
    assert lib.rf_sh_entries_workspace_bytes(1, 0) == 48 and lib.rf_sh_entries_workspace_bytes(chunk + 1, 3) == 1536

    # argument checks come before anything touches the device
    d = np.zeros(64).ctypes.data
    calls = {
        "forward": lambda deg, s, p: lib.rf_sh_entries_forward(deg, 4, s, 2, p, d, d, 48, d, d, None),
        "backward_coeffs": lambda deg, s, p: lib.rf_sh_entries_backward_coeffs(deg, 4, s, 2, p, d, d, d, d, d, d, d,
                                                                              1 << 20, None),
        "backward_directions": lambda deg, s, p: lib.rf_sh_entries_backward_directions(deg, 4, s, 2, p, d, d, 48, d, d,
                                                                                      d, d, None),
    }
    for name, call in calls.items():
        assert call(1, -1, d) == -1 and "negative entry count" in _lib.last_error(), name
        assert _lib.last_error().startswith("rf_sh_entries_" + name)
        assert call(1, 5, None) == -1 and "null pointer" in _lib.last_error(), name
        assert call(4, 5, d) == -1 and "the degree must be 0 .. 3" in _lib.last_error(), name
    assert lib.rf_sh_entries_forward(3, 4, 5, 2, d, d, d, 47, d, d, None) == -1 and "pitch" in _lib.last_error()
    assert lib.rf_sh_entries_backward_coeffs(1, 4, 5, 2, d, d, d, d, d, d, d, d, 8, None) == -2
    assert "workspace" in _lib.last_error()


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_torch_backend_matches_the_loop(degree):
    """Float64 sums of at most 16 products of numbers below 6: 1e-13 covers every order of addition."""
    seg, index, cells, coeffs, directions = _small_case(degree, seed=10 + degree)
    want, pre = _loop(OFFSETS, cells, coeffs, directions, degree)
    assert (pre < -0.1).any() and (pre > 0.1).any() and (want == 0).any()                     # clamped channels
    for backend in (None, "torch"):
        got = sh_entries(seg, index, coeffs, directions, backend=backend)
        assert got.dtype == torch.float64 and got.shape == (8, 3)
        np.testing.assert_allclose(got.numpy(), want, rtol=0, atol=1e-13)
        assert bool((got[torch.from_numpy(pre < 0)] == 0).all())
    # a [2, 3, 6] rays slice, float32 coefficients, float16 coefficients
    rays = torch.cat([torch.zeros(6, 3, dtype=torch.float64), directions], dim=-1).reshape(2, 3, 6)
    assert torch.equal(sh_entries(seg, index, coeffs, rays[..., 3:6]), got)
    got32 = sh_entries(seg, index, coeffs.float(), directions)
    assert got32.dtype == torch.float32
    np.testing.assert_allclose(got32.numpy(), want, rtol=0, atol=1e-5)
    assert sh_entries(seg, index, coeffs.half(), directions).dtype == torch.float16


@pytest.mark.parametrize("degree", [1, 2, 3])
def test_gradcheck(degree):
    seg, index, cells, coeffs, directions = _small_case(degree, seed=20 + degree)
    _, pre = _loop(OFFSETS, cells, coeffs, directions, degree)
    assert np.abs(pre).min() > 1e-3 and (pre < -0.1).any() and (pre > 0.1).any()
    coeffs, directions = coeffs.requires_grad_(True), directions.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda c, d: sh_entries(seg, index, c, d), (coeffs, directions))
    # the gradient of the clamp is zero where the colour is zero; cell 4 has no entry; rays 0, 2 and 5 have none
    sh_entries(seg, index, coeffs, directions).sum().backward()
    assert bool((coeffs.grad[1, 0::3] == 0).all()) and bool((coeffs.grad[4] == 0).all())
    assert bool((coeffs.grad[0] != 0).any()) and bool((directions.grad[[0, 2, 5]] == 0).all())
    assert bool((directions.grad[[1, 3, 4]] != 0).any())
    # the gradient of a direction is at right angles to it: the colour does not depend on its length
    along = (directions.grad * directions.detach()).sum(-1)
    assert float(along.abs().max()) <= 1e-12


def test_degree_zero_has_no_direction_gradient():
    seg, index, cells, coeffs, directions = _small_case(0, seed=30)
    directions.requires_grad_(True)
    sh_entries(seg, index, coeffs.requires_grad_(True), directions).sum().backward()
    assert bool((directions.grad == 0).all()) and bool((coeffs.grad != 0).any())


def test_validation():
    seg, index, cells, coeffs, directions = _small_case(2, seed=31)
    assert sh_entries(seg, index, coeffs, directions).shape == (8, 3)
    for backend in ("cuda", "HIP", ""):
        with pytest.raises(ValueError, match="backend must be None, 'hip' or 'torch'"):
            sh_entries(seg, index, coeffs, directions, backend=backend)
    with pytest.raises(RuntimeError, match="the kernel takes float32 CUDA coeffs"):
        sh_entries(seg, index, coeffs.float(), directions, backend="hip")
    with pytest.raises(RuntimeError, match="index must be the CellEntries"):
        sh_entries(seg, {"cells": seg["cells"]}, coeffs, directions)
    for bad in (coeffs[:, :26], coeffs[:, :4], torch.zeros(NUM_CELLS, 75, dtype=torch.float64), coeffs[:4],
                coeffs.reshape(-1), coeffs.to(torch.int64)):
        with pytest.raises(RuntimeError, match=r"(expected coeffs \[N, 3K\]|coeffs must have float16)"):
            sh_entries(seg, index, bad, directions)
    for bad in (directions[:5], directions[:, :2], directions.reshape(-1)[:17], directions.to(torch.int64)):
        with pytest.raises(RuntimeError, match=r"(expected directions \[R, 3\]|directions must be a floating-point)"):
            sh_entries(seg, index, coeffs, bad)
    with pytest.raises(RuntimeError, match=r"seg\['offsets'\] must be int64"):
        sh_entries({"offsets": OFFSETS.to(torch.int32)}, index, coeffs, directions)
    shorter = cell_entries({"cells": seg["cells"][:7]}, NUM_CELLS)                        # an index of another length
    with pytest.raises(RuntimeError, match=r"seg\['offsets'\]\[-1\] must be the number of entries of the index"):
        sh_entries(seg, shorter, coeffs, directions)
    with pytest.raises(RuntimeError, match="must live on the device of coeffs"):
        sh_entries(seg, index, coeffs, directions.to("meta"))


def _oracle_chain(foam_factory, degree, with_grad):
    """(rgba [R, 4] float64 of the chain over the oracle's own walk, coeffs, args of the oracle, rays, starts)."""
    fm, rays, starts, walk = S.image_case(foam_factory, sh_degree=degree)
    attributes = torch.from_numpy(fm["attributes"]).double()
    coeffs, density = attributes[:, :-1].clone(), attributes[:, -1].clone()
    if with_grad:
        coeffs.requires_grad_(True)
        density.requires_grad_(True)
    seg = {k: torch.from_numpy(walk[k]) for k in ("offsets", "cells", "t_enter", "t_exit")}
    index = cell_entries(seg, attributes.size(0))
    sigma = gather_cells(index, density)
    rgb = sh_entries(seg, index, coeffs, torch.from_numpy(rays)[..., 3:6].double())
    rgb = rgb * (sigma.detach() > 1e-6).unsqueeze(-1)                                      # the tracer's density gate
    out = composite_entries(seg, sigma, rgb)
    args = (degree, fm["points"], fm["attributes"], fm["point_adjacency"], fm["point_adjacency_offsets"])
    return out, coeffs, rgb, args, rays, starts


@pytest.mark.parametrize("degree", [1, 2, 3])
def test_chain_reproduces_the_oracles_trace_forward(foam_factory, degree):
    """The bar of test_reproduces_trace_forward: 1e-4 absolute on the oracle's fp32 rgba."""
    from oracle import oracle as O

    out, _, rgb, args, rays, starts = _oracle_chain(foam_factory, degree, with_grad=False)
    want = O.trace_forward(*args, rays, starts)["rgba"].reshape(-1, 4).astype(np.float64)
    worst = float(np.abs(out.numpy() - want).max())
    print("degree %d: largest |chain - oracle trace_forward| %.3g; %d of %d colour channels clamped"
          % (degree, worst, int((rgb == 0).sum()), rgb.numel()))
    assert out.shape == want.shape and want[:, 3].max() > 0.5 and want[:, :3].max() > 0.3
    assert worst <= 1e-4


def test_chain_reproduces_the_oracles_trace_backward(foam_factory):
    """Autograd of sum(rgba^2) through gather_cells -> sh_entries -> composite_entries in float64 at degree 2, against
    the SH columns of the oracle's trace_backward attribute gradient for the same loss: helpers.grad_close, DESIGN
    section 2's bar for gradients."""
    from oracle import oracle as O

    out, coeffs, rgb, args, rays, starts = _oracle_chain(foam_factory, 2, with_grad=True)
    out.square().sum().backward()
    fwd = O.trace_forward(*args, rays, starts)
    ref = O.trace_backward(*args, rays, starts, fwd["rgba"], 2.0 * fwd["rgba"], num_threads=1)["attr_grad"][:, :-1]
    ok, rel, worst = H.grad_close(coeffs.grad.numpy(), ref)
    print("degree 2: SH attribute gradient against the oracle: relative L2 %.3g, worst element at %.3g of its bound; "
          "largest |reference| %.3g; %d colour channels clamped"
          % (rel, worst, np.abs(ref).max(), int((rgb == 0).sum())))
    assert coeffs.grad.shape == ref.shape and np.abs(ref).max() > 1e-3
    assert ok, (rel, worst)


def test_example_at_toy_size():
    from examples.sh_shading import main

    out = main(num_points=400, width=12, height=9, steps=12, device="cpu", log=lambda *_: None)
    print("example: loss %.5g -> %.5g" % (out["first"], out["last"]))
    assert np.isfinite(out["last"]) and out["last"] < 0.7 * out["first"]
