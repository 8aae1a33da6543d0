"""The walk by cell on the GPU (rf_cell_reduce.hip): the kernels against the float64 torch backend on
hand-built indices whose list lengths are taken from the chunk a wave owns, so that lists begin, end and run through
chunk boundaries where that can go wrong; exact counts; bitwise reproducibility; and the real walk against
trace_forward's contribution and against float64 autograd of table[cells].

The bar is the project's for a result summed in double and rounded once to float32: rtol = 2e-7, atol = 1e-7 (half a
float32 ulp is 6e-8 relative).  Values lie in -1 .. 1, so that atol is not a free pass."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.helpers import cell_list_lengths as _lengths
from tests import segments_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RTOL, ATOL = 2e-7, 1e-7


def _chunk():
    from radfoam_amd import _lib

    k = int(_lib.load().rf_reduce_entries_chunk())
    assert k >= 256 and k % 64 == 0
    return k


def _index(lengths, seed):
    """(index, cells): entries scattered through the list, not cell by cell."""
    import radfoam

    cells = np.repeat(np.arange(len(lengths)), lengths)
    np.random.default_rng(seed).shuffle(cells)
    cells = torch.from_numpy(cells.astype(np.int64)).to(torch.uint32).to(DEV)
    return radfoam.cell_entries({"cells": cells}, len(lengths)), cells


def _values(total, channels, seed):
    shape = (total,) if channels is None else (total, channels)
    return torch.from_numpy(np.random.default_rng(seed).uniform(-1.0, 1.0, size=shape).astype(np.float32)).to(DEV)


def _close(name, got, want):
    got, want = got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy()
    err = np.abs(got - want)
    bound = ATOL + RTOL * np.abs(want)
    print("%s: largest |kernel - float64 torch backend| %.3g, at %.3g of its bound; largest |reference| %.3g"
          % (name, err.max(initial=0.0), (err / bound).max(initial=0.0), np.abs(want).max(initial=0.0)))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=name)


def _check(name, index, values, lengths):
    import radfoam

    out = radfoam.reduce_entries(index, values)
    assert out.dtype == torch.float32 and out.is_cuda and out.shape == (len(lengths),) + values.shape[1:]
    assert "ReduceEntries" in str(radfoam.reduce_entries(index, values.clone().requires_grad_(True)).grad_fn)
    ref = radfoam.reduce_entries(index, values.double(), backend="torch")
    torch.cuda.synchronize()
    _close(name, out, ref)
    empty = torch.tensor([n == 0 for n in lengths], device=DEV)
    assert bool((out[empty] == 0).all())
    return out


@pytest.mark.parametrize("channels", [None, 1, 3, 4, 5, 6, 7, 16])
def test_hand_built_index(channels):
    k = _chunk()
    lengths = _lengths(k)
    index, cells = _index(lengths, seed=40)
    assert index.cell_offsets.tolist() == np.concatenate([[0], np.cumsum(lengths)]).tolist()
    assert not bool((cells[1:].to(torch.int64) >= cells[:-1].to(torch.int64)).all())       # scattered
    values = _values(sum(lengths), channels, seed=41 + (channels or 0))
    out = _check("hand-built, C = %s" % channels, index, values, lengths)
    assert float(out.abs().max()) > 5                              # sums of up to 2K + 130 numbers


def test_counts_are_exact():
    import radfoam

    k = _chunk()
    lengths = _lengths(k)
    index, _ = _index(lengths, seed=42)
    ones = torch.ones(sum(lengths), dtype=torch.float32, device=DEV)
    assert radfoam.reduce_entries(index, ones).tolist() == [float(n) for n in lengths]
    both = radfoam.reduce_entries(index, torch.stack([ones, 2 * ones, 3 * ones], dim=-1))
    assert both.tolist() == [[float(n), 2.0 * n, 3.0 * n] for n in lengths]


def test_a_list_of_more_than_64_chunks_and_one_cell():
    """A list longer than the 64 chunks the second launch adds in one step, between two short ones; then N = 1 with a
    list of K + 5, N = 1 with S = 1, and S = 0."""
    import radfoam

    k = _chunk()
    lengths = [3, 70 * k + 5, 9, 0]
    index, _ = _index(lengths, seed=43)
    _check("70 chunks, C = 3", index, _values(sum(lengths), 3, seed=44), lengths)
    ones = torch.ones(sum(lengths), dtype=torch.float32, device=DEV)
    assert radfoam.reduce_entries(index, ones).tolist() == [float(n) for n in lengths]
    for n in (k + 5, 1):
        index, _ = _index([n], seed=45)
        _check("one cell, %d entries" % n, index, _values(n, 2, seed=46), [n])
    none, _ = _index([0], seed=47)
    out = radfoam.reduce_entries(none, torch.zeros((0, 2), dtype=torch.float32, device=DEV))
    assert out.shape == (1, 2) and out.dtype == torch.float32 and out.is_cuda and bool((out == 0).all())
    assert radfoam.gather_cells(none, torch.ones(1, device=DEV)).shape == (0,)


def test_bitwise_reproducible():
    import radfoam

    k = _chunk()
    lengths = _lengths(k)
    index, cells = _index(lengths, seed=48)
    values = _values(sum(lengths), 5, seed=49)
    first = radfoam.reduce_entries(index, values)
    assert torch.equal(first, radfoam.reduce_entries(index, values))
    assert torch.equal(first, radfoam.reduce_entries(radfoam.cell_entries({"cells": cells}, len(lengths)), values))
    grads = []
    for _ in range(2):
        table = _values(len(lengths), 5, seed=50).requires_grad_(True)
        looked_up = radfoam.gather_cells(index, table)
        assert torch.equal(looked_up, table.detach()[cells.to(torch.int64)])
        looked_up.backward(values)
        grads.append(table.grad)
    assert grads[0].dtype == torch.float32 and torch.equal(grads[0], grads[1]) and torch.equal(grads[0], first)


def _device_inputs(fm, rays, starts):
    p, a, adj, off = H.to_torch_foam(fm, DEV)
    r = torch.from_numpy(np.ascontiguousarray(rays)).to(DEV)
    s = torch.from_numpy(np.ascontiguousarray(starts, dtype=np.uint32)).to(DEV)
    return p, a, adj, off, r, s


def _real_walk(foam_factory):
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
    """The compositing weights of the pipeline's own walk, summed per cell by the kernel, against the pipeline's
    trace_forward(return_contribution=True): DESIGN section 2's bar for scatter outputs, 1e-3 per element and 1e-5
    relative L2, over every cell."""
    import radfoam
    from examples.cell_statistics import entry_weights

    pipe, inputs, seg, index = _real_walk(foam_factory)
    ref = pipe.trace_forward(*inputs, return_contribution=True)["contribution"].reshape(-1).double()
    sigma = inputs[1][:, -1].float()[index.cells]
    weights, _ = entry_weights(seg, sigma)
    got = radfoam.reduce_entries(index, weights.float())
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and got.is_cuda
    err = (got.double() - ref).abs()
    rel = float((err ** 2).sum().sqrt() / (ref ** 2).sum().sqrt())
    print("%d entries; %d cells of non-zero contribution, the largest %.3g; largest difference %.3g, at %.3g of its "
          "bound; relative L2 %.3g, at %.3g of its bound"
          % (index.cells.numel(), int((ref != 0).sum()), float(ref.max()), float(err.max()), float(err.max()) / 1e-3,
             rel, rel / 1e-5))
    assert got.shape == ref.shape and int((ref != 0).sum()) > 500 and float(ref.max()) > 1
    assert float(err.max()) <= 1e-3 and rel <= 1e-5


def test_real_walk_gradients_of_the_tables(foam_factory):
    """A loss on composite_entries' output, back through gather_cells into a density [N] and a colour [N, 3] per cell:
    the kernels' chain in float32 against float64 autograd of table[cells] under the torch backend."""
    import radfoam

    _, inputs, seg, index = _real_walk(foam_factory)
    num_cells = inputs[0].size(0)
    rng = np.random.default_rng(51)
    density0 = torch.from_numpy(rng.uniform(0.0, 3.0, size=num_cells).astype(np.float32)).to(DEV)
    colour0 = torch.from_numpy(rng.uniform(-1.0, 1.0, size=(num_cells, 3)).astype(np.float32)).to(DEV)
    g = torch.from_numpy(rng.normal(size=(3072, 4)).astype(np.float32)).to(DEV)

    density, colour = density0.clone().requires_grad_(True), colour0.clone().requires_grad_(True)
    out = radfoam.composite_entries(seg, radfoam.gather_cells(index, density), radfoam.gather_cells(index, colour))
    assert out.dtype == torch.float32 and "CompositeEntries" in str(out.grad_fn)
    out.backward(g)
    density64, colour64 = density0.double().requires_grad_(True), colour0.double().requires_grad_(True)
    ref = radfoam.composite_entries(seg, density64[index.cells], colour64[index.cells], backend="torch")
    ref.backward(g.double())
    torch.cuda.synchronize()
    for name, got, want in (("density.grad", density.grad, density64.grad), ("colour.grad", colour.grad, colour64.grad)):
        assert got.dtype == torch.float32 and got.shape == want.shape
        assert 0.05 < float(want.abs().max()) < 1e3, (name, float(want.abs().max()))
        _close(name, got, want)


def test_example_at_toy_size():
    from examples.cell_statistics import run

    out = run(num_points=2000, width=32, height=24, steps=3, log=lambda *_: None)
    contribution, error = out["contribution"], out["error"]
    print("contribution: sum %.4g, largest %.4g; prune %d, densify %d of %d cells; mse %.4g"
          % (float(contribution.sum()), float(contribution.max()), int(out["prune"].sum()), int(out["densify"].sum()),
             contribution.numel(), out["mse"]))
    assert contribution.shape == error.shape == (2000,) and contribution.dtype == torch.float32
    assert bool(torch.isfinite(contribution).all()) and bool((contribution >= 0).all()) and bool((error >= 0).all())
    # every ray's weights sum to its opacity: at most one per ray
    assert 0 < float(contribution.sum()) <= 32 * 24 * (1 + 1e-5)
    assert bool(out["prune"].any()) and bool(out["densify"].any()) and not bool((out["prune"] & out["densify"]).any())
