"""CPU: the walk by cell (radfoam.cell_entries, reduce_entries, gather_cells): the index on hand-built
cells against a stable sort, reduce_entries' torch backend against a float64 Python loop, both operators under gradcheck,
gather_cells against table[cells] and its autograd gradient, the oracle's per-cell contribution on a real walk,
validation, and the build lists."""
import os

import numpy as np
import pytest
import torch

import radfoam
import radfoam_amd
from radfoam import cell_entries, gather_cells, reduce_entries
from tests import segments_ref as S

# 12 cells: 0 and 1 empty (first), 5 and 6 empty (middle), 10 and 11 empty (last); cell 3 holds most of the entries
NUM_CELLS = 12


def _cells(seed=0, total=200):
    rng = np.random.default_rng(seed)
    few = rng.choice([2, 4, 7, 8, 9], size=total // 4)
    cells = np.concatenate([few, np.full(total - len(few), 3)])
    rng.shuffle(cells)
    return torch.from_numpy(cells.astype(np.int64))


def _loop(cells, values, num_cells):
    """out[c] = sum of values[e] over the entries of c, entry by entry in float64."""
    v = values.detach().double().numpy()
    out = np.zeros((num_cells,) + v.shape[1:])
    for e, c in enumerate(cells.tolist()):
        out[c] += v[e]
    return out


def test_public_surface():
    for name in ("CellEntries", "cell_entries", "reduce_entries", "gather_cells"):
        assert name in radfoam_amd.__all__ and name in radfoam.__all__
        assert getattr(radfoam, name) is getattr(radfoam_amd.cells, name)


def test_sources_are_built_but_not_part_of_the_source_hash():
    from radfoam_amd import _lib, build

    names = lambda paths: {os.path.basename(p) for p in paths}
    assert "rf_cell_reduce.hip" in names(build.EXTRA_SOURCES)
    assert {"radfoam_hip_cell_reduce.h", "rf_ray_sweep.hpp", "rf_cell_sweep.hpp"} <= names(build.EXTRA_HEADERS)
    assert not names(build.SOURCES + build.HEADERS) & {"rf_cell_reduce.hip", "radfoam_hip_cell_reduce.h",
                                                       "rf_cell_sweep.hpp"}
    assert not names(build.SOURCES + build.HEADERS) & names(build.EXTRA_SOURCES + build.EXTRA_HEADERS)
    lib = _lib.load()
    for name in ("rf_reduce_entries", "rf_reduce_entries_chunk", "rf_reduce_entries_workspace_bytes"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    chunk = lib.rf_reduce_entries_chunk()
    assert chunk >= 64 and chunk % 64 == 0
    # two rows of doubles per chunk
    assert lib.rf_reduce_entries_workspace_bytes(0, 3) == 0 and lib.rf_reduce_entries_workspace_bytes(-5, 3) == 0
    assert lib.rf_reduce_entries_workspace_bytes(1, 1) == 16
    assert lib.rf_reduce_entries_workspace_bytes(chunk, 3) == 48
    assert lib.rf_reduce_entries_workspace_bytes(chunk + 1, 3) == 96
    # argument checks come before anything touches the device
    dummy = np.zeros(64).ctypes.data
    assert lib.rf_reduce_entries(0, 5, None, None, None, 2, None, None, 0, None) == 0            # no cells: nothing to do
    assert lib.rf_reduce_entries(4, -1, dummy, dummy, dummy, 2, dummy, dummy, 1 << 20, None) == -1
    assert "negative entry count" in _lib.last_error()
    assert lib.rf_reduce_entries(-4, 5, dummy, dummy, dummy, 2, dummy, dummy, 1 << 20, None) == -1
    assert "negative cell count" in _lib.last_error()
    assert lib.rf_reduce_entries(4, 5, dummy, dummy, dummy, 0, dummy, dummy, 1 << 20, None) == -1
    assert "no channels" in _lib.last_error()
    assert lib.rf_reduce_entries(4, 5, dummy, dummy, dummy, 2, None, dummy, 1 << 20, None) == -1
    assert "null pointer" in _lib.last_error()


def test_index_is_the_stable_sort():
    cells = _cells()
    counts = np.bincount(cells.numpy(), minlength=NUM_CELLS)
    assert counts[[0, 1, 5, 6, 10, 11]].sum() == 0 and counts[3] >= 0.7 * len(cells) and (counts[[2, 4, 7, 8, 9]] > 0).all()
    for dtype in (torch.uint32, torch.int32, torch.int64):
        index = cell_entries({"cells": cells.to(dtype)}, NUM_CELLS)
        assert isinstance(index, radfoam.CellEntries) and index.num_cells == NUM_CELLS
        for t, n in ((index.cells, len(cells)), (index.entries, len(cells)), (index.sorted_cells, len(cells)),
                     (index.cell_offsets, NUM_CELLS + 1)):
            assert t.dtype == torch.int64 and t.shape == (n,)
        assert torch.equal(index.cells, cells)
        assert index.entries.tolist() == np.argsort(cells.numpy(), kind="stable").tolist()
        assert index.cell_offsets.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
        assert torch.equal(index.sorted_cells, cells[index.entries])
        off = index.cell_offsets.tolist()
        for c in range(NUM_CELLS):
            mine = index.entries[off[c]:off[c + 1]].tolist()
            assert mine == sorted(mine) and mine == np.nonzero(cells.numpy() == c)[0].tolist()


def test_index_without_entries_and_without_cells():
    index = cell_entries({"cells": torch.zeros(0, dtype=torch.uint32)}, 5)
    assert index.entries.shape == (0,) and index.cell_offsets.tolist() == [0] * 6
    out = reduce_entries(index, torch.zeros((0, 3), dtype=torch.float64))
    assert out.shape == (5, 3) and out.dtype == torch.float64 and bool((out == 0).all())
    assert gather_cells(index, torch.rand(5)).shape == (0,)
    none = cell_entries({"cells": torch.zeros(0, dtype=torch.int64)}, 0)
    assert none.cell_offsets.tolist() == [0] and reduce_entries(none, torch.zeros(0)).shape == (0,)


def test_index_validation():
    cells = _cells()
    bad = [
        (({"cells": cells.reshape(2, -1)}, NUM_CELLS), r"seg\['cells'\] must be a tensor \[S\]"),
        (({"cells": cells.tolist()}, NUM_CELLS), r"seg\['cells'\] must be a tensor \[S\]"),
        (({"cells": cells.float()}, NUM_CELLS), "must have uint32, int32 or int64 dtype"),
        (({"cells": cells.to(torch.int16)}, NUM_CELLS), "must have uint32, int32 or int64 dtype"),
        (({"cells": cells}, 9), r"must lie in 0 \.\. num_cells-1"),             # cell 9 is in use
        (({"cells": cells}, 0), r"must lie in 0 \.\. num_cells-1"),
        (({"cells": torch.tensor([0, -1, 2])}, 5), r"must lie in 0 \.\. num_cells-1"),
        (({"cells": cells}, -1), "num_cells must be a non-negative int"),
        (({"cells": cells}, 12.0), "num_cells must be a non-negative int"),
    ]
    for args, message in bad:
        with pytest.raises(RuntimeError, match=message):
            cell_entries(*args)
    assert cell_entries({"cells": cells}, 10).num_cells == 10                   # 9 is the largest cell in use


@pytest.mark.parametrize("channels", [None, 1, 3, 5])
def test_reduce_entries_matches_the_loop(channels):
    """Float64 sums of at most 200 numbers in -1 .. 1: 1e-13 covers every order of addition."""
    cells = _cells(seed=1)
    index = cell_entries({"cells": cells.to(torch.uint32)}, NUM_CELLS)
    shape = (len(cells),) if channels is None else (len(cells), channels)
    values = torch.from_numpy(np.random.default_rng(2).uniform(-1, 1, size=shape))
    want = _loop(cells, values, NUM_CELLS)
    for backend in (None, "torch"):
        out = reduce_entries(index, values, backend=backend)
        assert out.dtype == torch.float64 and out.shape == (NUM_CELLS,) + shape[1:]
        np.testing.assert_allclose(out.numpy(), want, rtol=0, atol=1e-13)
        assert bool((out[[0, 1, 5, 6, 10, 11]] == 0).all()) and float(out[3].abs().max()) > 0
    # float32 values: summed in float64, rounded once
    out32 = reduce_entries(index, values.float())
    assert out32.dtype == torch.float32
    want32 = _loop(cells, values.float(), NUM_CELLS)
    np.testing.assert_allclose(out32.numpy(), want32, rtol=2e-7, atol=1e-7)
    ones = reduce_entries(index, torch.ones(len(cells)))
    assert ones.tolist() == np.bincount(cells.numpy(), minlength=NUM_CELLS).tolist()


def test_gradcheck_and_the_lookup():
    cells = _cells(seed=3, total=40)
    index = cell_entries({"cells": cells}, NUM_CELLS)
    rng = np.random.default_rng(4)
    for shape in ((), (3,)):
        values = torch.from_numpy(rng.uniform(-1, 1, size=(len(cells),) + shape)).requires_grad_(True)
        table = torch.from_numpy(rng.uniform(-1, 1, size=(NUM_CELLS,) + shape)).requires_grad_(True)
        assert torch.autograd.gradcheck(lambda v: reduce_entries(index, v), (values,))
        assert torch.autograd.gradcheck(lambda t: gather_cells(index, t), (table,))
        for dtype in (torch.float64, torch.float32):
            leaf = table.detach().to(dtype).requires_grad_(True)
            plain = table.detach().to(dtype).requires_grad_(True)
            got, want = gather_cells(index, leaf), plain[cells]
            assert got.dtype == dtype and torch.equal(got, want) and "GatherCells" in str(got.grad_fn)
            g = torch.from_numpy(rng.normal(size=tuple(want.shape))).to(dtype)
            got.backward(g)
            want.backward(g)
            # float64: sums of at most 40 numbers in another order; float32: summed in double here, in float32 there
            tol = {"rtol": 0, "atol": 1e-13} if dtype == torch.float64 else {"rtol": 1e-5, "atol": 1e-5}
            assert leaf.grad.dtype == dtype and leaf.grad.shape == plain.grad.shape
            np.testing.assert_allclose(leaf.grad.numpy(), plain.grad.numpy(), **tol)
            assert bool((leaf.grad[[0, 1, 5, 6, 10, 11]] == 0).all())
        # the gradient of reduce_entries is the lookup
        leaf = values.detach().clone().requires_grad_(True)
        g = torch.from_numpy(rng.normal(size=(NUM_CELLS,) + shape))
        reduce_entries(index, leaf).backward(g)
        assert torch.allclose(leaf.grad, g[cells], rtol=0, atol=0)


def test_operator_validation():
    cells = _cells(total=40)
    index = cell_entries({"cells": cells}, NUM_CELLS)
    values, table = torch.rand(40, 3), torch.rand(NUM_CELLS, 3)
    assert reduce_entries(index, values).shape == (NUM_CELLS, 3) and gather_cells(index, table).shape == (40, 3)
    for fn, good in ((reduce_entries, values), (gather_cells, table)):
        for backend in ("cuda", "HIP", ""):
            with pytest.raises(ValueError, match="backend must be None, 'hip' or 'torch'"):
                fn(index, good, backend=backend)
        with pytest.raises(RuntimeError, match="the kernel takes float32 CUDA"):
            fn(index, good, backend="hip")
        with pytest.raises(RuntimeError, match="index must be the CellEntries"):
            fn({"cells": cells}, good)
        with pytest.raises(RuntimeError, match="must have float32 or float64 dtype"):
            fn(index, good.to(torch.float16))
        with pytest.raises(RuntimeError, match="must have float32 or float64 dtype"):
            fn(index, good.to(torch.int64))
        for shape in ((good.size(0) - 1, 3), (good.size(0), 3, 1), (good.size(0), 0), ()):
            with pytest.raises(RuntimeError, match=r"expected (values \[S\] or \[S, C\]|table \[N\] or \[N, C\])"):
                fn(index, torch.zeros(shape))


def test_contribution_against_the_oracle(foam_factory):
    """oracle.trace_forward(return_contribution=True) on the 64x48 frame at SH 0 against reduce_entries of the
    compositing weights of composite_entries' definition, in float64 over the oracle's own walk with density[cells].  The
    bar is DESIGN section 2's for scatter outputs: 1e-3 per element and 1e-5 relative L2, over every cell.  Measured:
    largest difference 2.6e-6, relative L2 1.0e-7, 815 cells of non-zero contribution, the largest 16.8."""
    from oracle import oracle as O

    fm, rays, starts, walk = S.image_case(foam_factory, sh_degree=0)
    num_cells = fm["points"].shape[0]
    ref = O.trace_forward(fm["sh_degree"], fm["points"], fm["attributes"], fm["point_adjacency"],
                          fm["point_adjacency_offsets"], rays, starts, return_contribution=True)
    ref = ref["contribution"].reshape(-1).astype(np.float64)

    off, cells = walk["offsets"], walk["cells"].astype(np.int64)
    t_enter, t_exit = walk["t_enter"].astype(np.float64), walk["t_exit"].astype(np.float64)
    dt = np.where(np.isinf(t_exit), 0.0, np.maximum(np.where(np.isinf(t_exit), 0.0, t_exit) - t_enter, 0.0))
    x = fm["attributes"][:, -1].astype(np.float64)[cells] * dt
    weights = np.zeros(len(cells))
    for r in range(len(off) - 1):                                 # the definition, ray by ray
        e = slice(off[r], off[r + 1])
        weights[e] = np.exp(-(np.cumsum(x[e]) - x[e])) * -np.expm1(-x[e])

    index = cell_entries({"cells": torch.from_numpy(walk["cells"])}, num_cells)
    lengths = (index.cell_offsets[1:] - index.cell_offsets[:-1]).numpy()
    got = reduce_entries(index, torch.from_numpy(weights)).numpy()
    err = np.abs(got - ref)
    rel = np.sqrt((err ** 2).sum() / (ref ** 2).sum())
    print("%d entries over %d of %d cells, longest list %d, median %d; %d cells of non-zero contribution, the largest "
          "%.3g; largest difference %.3g, relative L2 %.3g"
          % (len(cells), (lengths > 0).sum(), num_cells, lengths.max(), np.median(lengths[lengths > 0]),
             (ref != 0).sum(), ref.max(), err.max(), rel))
    assert got.shape == ref.shape == (num_cells,) and lengths.max() == len(off) - 1 == 3072
    assert (ref != 0).sum() > 500 and ref.max() > 1
    assert (got[lengths == 0] == 0).all()
    assert err.max() <= 1e-3 and rel <= 1e-5
