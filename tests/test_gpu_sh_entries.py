"""radfoam.sh_entries on the GPU (rf_sh_entries.hip): the forward bit for bit against the tracer on probe
rays, and on every entry of a real walk against the float64 torch backend; both gradients on a hand-built walk whose
cell lists are taken from the chunk a wave owns and whose rays from the steps a wave takes, against float64 autograd;
exact zeros, bitwise reproducibility, edge cases; and the chain gather_cells -> sh_entries -> composite_entries against
trace_forward and trace_backward.

Every bound is derived from counts of fp32 roundings (u = 2^-24), none from what the kernels give:
    forward       (K + 14) u (0.5 + sum_k |coeffs[cell, 3k + c]|): K roundings of the chain; up to 5 inside a basis
                  value with sup |Y_k| <= 0.75; 3 of the normalisation times sup |grad Y_k| <= 3
    coeffs.grad   16 u sum over the cell's entries of |m g[e, c]| + u |want|: the same counts for the basis value, one
                  rounding of the product, one final rounding of the double sum
    directions.grad   32 u 3 sum over the ray's entries of sum_{k, c} |m g[e, c] coeffs[cell, 3k + c]| / |d|: a chain of
                  at most 32 roundings, sup |grad Y_k| <= 3
Each test prints observed over bound."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.helpers import cell_list_lengths_long as _lengths
from tests import segments_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
_WALKS = {}


def _chunk():
    from radfoam_amd import _lib

    k = int(_lib.load().rf_reduce_entries_chunk())
    assert k >= 256 and k % 64 == 0
    return k


def _hand_built(degree, seed):
    """A walk that no tracer made: cells scattered through the list with the list lengths above; rays of 300 entries
    (several steps of a wave), then 0, 1, 63, 64, 65 and 129 in turn, padded with empty rays to a [H, 7] frame.
    Coefficients whose colours stay 0.1 clear of the clamp on either side, so that float32 and float64 agree on the
    mask; cells 2, 9 and 14 are pushed below it."""
    import radfoam

    rng = np.random.default_rng(seed)
    lengths = _lengths(_chunk())
    total, num_cells = sum(lengths), len(lengths)
    cells = np.repeat(np.arange(num_cells), lengths)
    rng.shuffle(cells)
    counts = [300]
    while sum(counts) < total:
        counts += [0, 1, 63, 64, 65, 129]
    counts = np.array(counts, dtype=np.int64)
    counts[-1] -= counts.sum() - total
    while counts[-1] < 0:                                          # the last rays of the cycle: cut back to the total
        counts[-2] += counts[-1]
        counts = counts[:-1]
    counts = np.concatenate([counts, np.zeros((-len(counts)) % 7 + 7, dtype=np.int64)])
    assert counts.sum() == total and (counts >= 0).all() and len(counts) % 7 == 0
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)])).to(DEV)
    cells = torch.from_numpy(cells.astype(np.int64)).to(DEV)
    seg = {"offsets": offsets, "cells": cells.to(torch.uint32)}
    index = radfoam.cell_entries(seg, num_cells)
    num_basis = (degree + 1) ** 2
    coeffs = rng.uniform(-1.0, 1.0, size=(num_cells, 3 * num_basis)) * (0.4 / (0.75 * num_basis))     # |sum| <= 0.4
    coeffs[2, :3] -= 5.0                                           # 0.5 - 5 C0 = -0.91: all three channels clamped
    coeffs[9, 1] -= 5.0
    coeffs[14, 2] -= 5.0
    rays = np.zeros((len(counts) // 7, 7, 6), dtype=np.float32)
    rays[..., 3:] = rng.normal(size=rays.shape[:-1] + (3,)) * rng.uniform(0.5, 3.0, size=rays.shape[:-1] + (1,))
    grad = rng.normal(size=(total, 3)).astype(np.float32)
    return {"seg": seg, "index": index, "lengths": lengths, "counts": counts, "cells": cells,
            "coeffs": torch.from_numpy(coeffs.astype(np.float32)).to(DEV), "rays": torch.from_numpy(rays).to(DEV),
            "grad": torch.from_numpy(grad).to(DEV)}


def _both_backwards(case):
    """((rgb, coeffs.grad, directions.grad) of the kernels, the same of the float64 torch backend)."""
    import radfoam

    out = []
    for dtype, backend in ((torch.float32, None), (torch.float64, "torch")):
        coeffs = case["coeffs"].to(dtype).clone().requires_grad_(True)
        rays = case["rays"].to(dtype).clone().requires_grad_(True)
        directions = rays[..., 3:6]                                # the slice of the frame's rays, as it is
        rgb = radfoam.sh_entries(case["seg"], case["index"], coeffs, directions, backend=backend)
        assert rgb.dtype == dtype and rgb.is_cuda and rgb.shape == (case["cells"].numel(), 3)
        if backend is None:
            assert "ShEntries" in str(rgb.grad_fn)
        rgb.backward(case["grad"].to(dtype))
        assert coeffs.grad.dtype == dtype and coeffs.grad.shape == coeffs.shape
        assert rays.grad.dtype == dtype and rays.grad.shape == rays.shape and bool((rays.grad[..., :3] == 0).all())
        out.append((rgb.detach(), coeffs.grad, rays.grad[..., 3:6].reshape(-1, 3)))
    torch.cuda.synchronize()
    return out


def _ratio(name, got, want, bound):
    err = (got.double() - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print("%s: largest |kernel - float64 torch backend| %.3g, observed over bound %.3g; largest |reference| %.3g"
          % (name, float(err.max()) if err.numel() else 0.0, ratio, float(want.abs().max()) if err.numel() else 0.0))
    return bool((err <= bound).all())


def _masked_grad(case, rgb64):
    return torch.where(rgb64 > 0, case["grad"].double(), torch.zeros_like(rgb64)).abs()         # |m g| [S, 3]


def _device_inputs(fm, rays, starts):
    p, a, adj, off = H.to_torch_foam(fm, DEV)
    r = torch.from_numpy(np.ascontiguousarray(rays)).to(DEV)
    s = torch.from_numpy(np.ascontiguousarray(starts, dtype=np.uint32)).to(DEV)
    return p, a, adj, off, r, s


def _real_walk(foam_factory, degree):
    """The pipeline's own walk of image_case at ``degree``, its index, and the colours of all its entries: once."""
    import radfoam

    if degree not in _WALKS:
        fm, rays, starts, _ = S.image_case(foam_factory, sh_degree=degree)
        inputs = _device_inputs(fm, rays, starts)
        pipe = radfoam.create_pipeline(degree)
        seg = pipe.trace_segments(*inputs)
        index = radfoam.cell_entries(seg, inputs[0].size(0))
        coeffs = inputs[1][:, :-1]                                 # a column slice of the attributes, read in place
        assert not coeffs.is_contiguous()
        rgb = radfoam.sh_entries(seg, index, coeffs, inputs[4][..., 3:6])
        assert rgb.dtype == torch.float32 and rgb.is_cuda and rgb.shape == (index.cells.numel(), 3)
        _WALKS[degree] = (pipe, inputs, seg, index, coeffs, rgb)
    return _WALKS[degree]


@pytest.mark.parametrize("degree", [1, 2, 3])
def test_forward_is_the_tracers_colour_bit_for_bit(foam_factory, degree):
    """4096 entries of the walk, the first and the last among them.  Per entry a probe ray from the site of its cell in
    the direction of its ray (unnormalised), traced by trace_forward on the same foam with every density 1e6: the first
    cell is then exactly opaque (alpha rounds to 1.0f) and the pixel is that cell's colour to the bit.  Probes whose
    alpha is exactly 1 and whose num_intersections is 1 are kept (the tracer's outputs alone decide); at most 5 % may
    be left out (unbounded hull cells whose ray has no exit face)."""
    pipe, (p, a, adj, off, r, s), seg, index, coeffs, rgb = _real_walk(foam_factory, degree)
    total = index.cells.numel()
    rng = np.random.default_rng(60 + degree)
    pick = np.concatenate([[0, total - 1], 1 + rng.choice(total - 2, size=4094, replace=False)])
    pick = torch.from_numpy(pick.astype(np.int64)).to(DEV)
    entry_ray = torch.repeat_interleave(torch.arange(r.numel() // 6, device=DEV),
                                        seg["offsets"][1:] - seg["offsets"][:-1])[pick]
    cells = index.cells[pick]
    probes = torch.cat([p[cells], r.reshape(-1, 6)[entry_ray, 3:6]], dim=-1).contiguous()
    opaque = a.clone()
    opaque[:, -1] = 1e6
    out = pipe.trace_forward(p, opaque, adj, off, probes, cells.to(torch.uint32))
    torch.cuda.synchronize()
    rgba, hops = out["rgba"].reshape(-1, 4), out["num_intersections"].reshape(-1).to(torch.int64)
    keep = (rgba[:, 3] == 1.0) & (hops == 1)
    left_out = 1.0 - float(keep.double().mean())
    want, got = rgba[keep, :3].contiguous().view(torch.int32), rgb[pick][keep].contiguous().view(torch.int32)
    differ = int((want != got).any(dim=-1).sum())
    clamped = int((rgb[pick][keep] == 0).sum())
    print("degree %d: %d probes over %d distinct cells, %d kept, left out %.2f %%; %d probes whose bits differ; %d "
          "clamped channels among the kept" % (degree, pick.numel(), cells.unique().numel(), int(keep.sum()),
                                                100 * left_out, differ, clamped))
    assert left_out <= 0.05 and clamped >= 1
    assert differ == 0


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_forward_on_every_entry(foam_factory, degree):
    import radfoam

    _, (p, a, adj, off, r, s), seg, index, coeffs, rgb = _real_walk(foam_factory, degree)
    want = radfoam.sh_entries(seg, index, coeffs.double(), r[..., 3:6].double(), backend="torch")
    num_basis = (degree + 1) ** 2
    size = 0.5 + coeffs.double().abs().reshape(-1, num_basis, 3).sum(dim=1)                     # [N, 3]
    bound = (num_basis + 14) * U * size[index.cells]
    torch.cuda.synchronize()
    assert want.dtype == torch.float64 and (degree == 0 or int((want == 0).sum()) > 0) and float(want.max()) > 0.3
    assert _ratio("degree %d, %d entries, forward" % (degree, rgb.size(0)), rgb, want, bound)


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_gradients_on_a_hand_built_walk(degree):
    case = _hand_built(degree, seed=70 + degree)
    index, lengths, counts = case["index"], case["lengths"], case["counts"]
    assert index.cell_offsets.tolist() == np.concatenate([[0], np.cumsum(lengths)]).tolist()
    (rgb, grad_coeffs, grad_dirs), (rgb64, want_coeffs, want_dirs) = _both_backwards(case)
    num_basis = (degree + 1) ** 2
    total = rgb.size(0)
    # the two sides agree on the clamp, and it is in use
    assert torch.equal(rgb > 0, rgb64 > 0) and int((rgb == 0).sum()) > 100 and int((rgb > 0).sum()) > 100
    size = 0.5 + case["coeffs"].double().abs().reshape(-1, num_basis, 3).sum(dim=1)
    assert _ratio("degree %d, hand-built, forward" % degree, rgb, rgb64, (num_basis + 14) * U * size[index.cells])

    mg = _masked_grad(case, rgb64)
    per_cell = torch.zeros((len(lengths), 3), dtype=torch.float64, device=DEV).index_add(0, index.cells, mg)
    bound = 16 * U * per_cell.repeat(1, num_basis) + U * want_coeffs.abs()                  # column 3k + c: channel c
    assert float(want_coeffs.abs().max()) > 1
    assert _ratio("degree %d, hand-built, coeffs.grad" % degree, grad_coeffs, want_coeffs, bound)
    empty = torch.tensor([n == 0 for n in lengths], device=DEV)
    assert int(empty.sum()) == 5 and bool((grad_coeffs[empty] == 0).all())
    assert bool((grad_coeffs[2] == 0).all()) and bool((grad_coeffs[9, 1::3] == 0).all())       # clamped: no gradient

    weight = (mg * case["coeffs"].double().abs().reshape(-1, num_basis, 3).sum(dim=1)[index.cells]).sum(dim=-1)
    entry_ray = torch.repeat_interleave(torch.arange(len(counts), device=DEV), torch.from_numpy(counts).to(DEV))
    per_ray = torch.zeros(len(counts), dtype=torch.float64, device=DEV).index_add(0, entry_ray, weight)
    norm = case["rays"][..., 3:6].double().reshape(-1, 3).square().sum(-1).sqrt()
    bound = (32 * U * 3 * per_ray / norm).unsqueeze(-1).expand(-1, 3)
    assert _ratio("degree %d, hand-built, directions.grad" % degree, grad_dirs, want_dirs, bound)
    none = torch.from_numpy(counts == 0).to(DEV)
    assert int(none.sum()) > 7 and bool((grad_dirs[none] == 0).all())
    if degree == 0:
        assert bool((grad_dirs == 0).all()) and bool((want_dirs == 0).all())
    else:
        assert float(want_dirs.abs().max()) > 0.1 and counts.max() == 300 and total % 64 != 0


def test_bitwise_reproducible():
    import radfoam

    case = _hand_built(3, seed=80)
    first, _ = _both_backwards(case)
    again = radfoam.cell_entries(case["seg"], len(case["lengths"]))                          # and through a new index
    coeffs, rays = case["coeffs"].clone().requires_grad_(True), case["rays"].clone().requires_grad_(True)
    rgb = radfoam.sh_entries(case["seg"], again, coeffs, rays[..., 3:6])
    rgb.backward(case["grad"])
    torch.cuda.synchronize()
    assert torch.equal(rgb.detach().view(torch.int32), first[0].view(torch.int32))
    assert torch.equal(coeffs.grad.view(torch.int32), first[1].view(torch.int32))
    assert torch.equal(rays.grad[..., 3:6].reshape(-1, 3).contiguous().view(torch.int32),
                       first[2].contiguous().view(torch.int32))
    assert float(first[1].abs().max()) > 1 and float(first[2].abs().max()) > 0.1


def test_edge_cases():
    import radfoam

    def run(counts, cells, num_cells, degree=2):
        seg = {"offsets": torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int64, device=DEV),
               "cells": torch.tensor(cells, dtype=torch.int64, device=DEV)}
        index = radfoam.cell_entries(seg, num_cells)
        gen = torch.Generator().manual_seed(len(cells))
        coeffs = (torch.rand((num_cells, 3 * (degree + 1) ** 2), generator=gen) - 0.5).mul(0.1).to(DEV)
        coeffs.requires_grad_(True)
        dirs = (torch.rand((len(counts), 3), generator=gen) + 0.1).to(DEV).requires_grad_(True)
        rgb = radfoam.sh_entries(seg, index, coeffs, dirs)
        assert rgb.shape == (len(cells), 3) and rgb.dtype == torch.float32 and rgb.is_cuda
        rgb.sum().backward()
        want = radfoam.sh_entries(seg, index, coeffs.detach().double(), dirs.detach().double(), backend="torch")
        torch.cuda.synchronize()
        assert coeffs.grad.shape == coeffs.shape and dirs.grad.shape == dirs.shape
        assert torch.allclose(rgb.detach().double(), want, rtol=0, atol=1e-5)
        return coeffs.grad, dirs.grad

    grad_coeffs, grad_dirs = run([0, 0, 0], [], 4)                 # S = 0
    assert bool((grad_coeffs == 0).all()) and bool((grad_dirs == 0).all())
    grad_coeffs, grad_dirs = run([], [], 4)                        # R = 0
    assert bool((grad_coeffs == 0).all()) and grad_dirs.shape == (0, 3)
    grad_coeffs, grad_dirs = run([2, 0, 70], [0] * 72, 1)          # N = 1
    assert abs(float(grad_coeffs[0, 0]) - 72 * 0.28209479177387814) < 1e-4 and bool((grad_dirs[1] == 0).all())
    assert bool((grad_dirs[[0, 2]] != 0).any())

    seg = {"offsets": torch.tensor([0, 2], dtype=torch.int64), "cells": torch.tensor([0, 1], dtype=torch.int64)}
    with pytest.raises(RuntimeError, match="the kernel takes float32 CUDA coeffs"):
        radfoam.sh_entries(seg, radfoam.cell_entries(seg, 2), torch.zeros(2, 12), torch.ones(1, 3), backend="hip")
    with pytest.raises(RuntimeError, match="must live on the device of coeffs"):
        radfoam.sh_entries(seg, radfoam.cell_entries(seg, 2), torch.zeros(2, 12, device=DEV), torch.ones(1, 3))


def _chain(seg, index, density, coeffs, directions):
    import radfoam

    sigma = radfoam.gather_cells(index, density)
    rgb = radfoam.sh_entries(seg, index, coeffs, directions)
    rgb = rgb * (sigma.detach() > 1e-6).unsqueeze(-1)                                      # the tracer's density gate
    return radfoam.composite_entries(seg, sigma, rgb)


@pytest.mark.parametrize("degree", [1, 2, 3])
def test_chain_reproduces_trace_forward(foam_factory, degree):
    """The bar of tests/test_gpu_composite_entries.py::test_reproduces_trace_forward, which covers degree 0 only: 1e-4
    absolute on trace_forward's fp32 rgba."""
    pipe, (p, a, adj, off, r, s), seg, index, coeffs, _ = _real_walk(foam_factory, degree)
    got = _chain(seg, index, a[:, -1].contiguous(), coeffs, r[..., 3:6]).double()
    want = pipe.trace_forward(p, a, adj, off, r, s)["rgba"].reshape(-1, 4).double()
    torch.cuda.synchronize()
    worst = float((got - want).abs().max())
    print("degree %d: largest |chain - trace_forward| %.3g" % (degree, worst))
    assert got.shape == want.shape and float(want[:, 3].max()) > 0.5 and float(want[:, :3].max()) > 0.3
    assert worst <= 1e-4


def test_chain_reproduces_trace_backward(foam_factory):
    """Autograd of sum(rgba^2) through the chain at degree 2 against the SH columns of trace_backward's attribute
    gradient for the same loss: helpers.grad_close, DESIGN section 2's bar for gradients."""
    pipe, (p, a, adj, off, r, s), seg, index, _, _ = _real_walk(foam_factory, 2)
    coeffs = a[:, :-1].clone().requires_grad_(True)
    density = a[:, -1].clone().requires_grad_(True)
    _chain(seg, index, density, coeffs, r[..., 3:6]).square().sum().backward()
    fwd = pipe.trace_forward(p, a, adj, off, r, s)["rgba"]
    ref = pipe.trace_backward(p, a, adj, off, r, s, fwd, 2.0 * fwd)["attr_grad"][:, :-1]
    torch.cuda.synchronize()
    ok, rel, worst = H.grad_close(coeffs.grad.cpu().numpy(), ref.cpu().numpy())
    print("degree 2: SH attribute gradient against trace_backward: relative L2 %.3g, worst element at %.3g of its "
          "bound; largest |reference| %.3g" % (rel, worst, float(ref.abs().max())))
    assert coeffs.grad.shape == ref.shape and float(ref.abs().max()) > 1e-3
    assert ok, (rel, worst)


def test_example_on_the_device():
    from examples.sh_shading import main

    out = main(num_points=2000, width=32, height=24, steps=12, log=lambda *_: None)
    print("example: loss %.5g -> %.5g" % (out["first"], out["last"]))
    assert np.isfinite(out["last"]) and out["last"] < 0.7 * out["first"]
