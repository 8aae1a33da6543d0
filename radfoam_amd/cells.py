"""The exported walk (``Pipeline.trace_segments``) BY CELL: which entries scan a cell, the sum per cell of a per-entry
quantity, and the lookup of a per-cell table whose backward is that sum.

``cell_entries`` transposes a walk once: a stable sort of its entries by cell.  ``reduce_entries`` sums a per-entry
quantity per cell through that index, and ``gather_cells`` is ``table[cells]`` with ``reduce_entries`` as its backward.
For float32 tensors on the device the sum is the kernel of rf_cell_reduce.hip: work dealt by sorted positions and never
by cells (the start cell of a camera frame holds one entry of every ray), sums in double, one rounding to float32, no
atomics, the same bits from call to call.  Everything else is a float64 ``index_add``.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from .segments import _choose_backend


class CellEntries(NamedTuple):
    """The walk transposed (``cell_entries``).  Every tensor lives on the device of ``seg["cells"]``."""
    num_cells: int
    cells: torch.Tensor          # int64 [S]: seg["cells"] widened, the cell of every entry
    cell_offsets: torch.Tensor   # int64 [N+1]: cell c owns the positions cell_offsets[c] .. cell_offsets[c+1] - 1
    entries: torch.Tensor        # int64 [S]: the entry at every position; within a cell in ascending order
    sorted_cells: torch.Tensor   # int64 [S]: the cell of every position, cells[entries]: what the kernel reads


def cell_entries(seg, num_cells: int) -> CellEntries:
    """The walk ``seg`` (the dict ``Pipeline.trace_segments`` or ``trace_differentiable_segments`` returns; only
    ``seg["cells"]``, uint32 / int32 / int64 [S], is read) transposed for a foam of ``num_cells`` cells: per cell, the
    entries that scan it.

        entries[cell_offsets[c] : cell_offsets[c + 1]]   the entries of cell c, in ascending order

    so ``entries`` is the stable sort of 0 .. S-1 by cell.  Built once per walk with torch operations on the device of
    ``seg["cells"]`` (a stable sort, and the count and cumulative sum of the cells as one ``searchsorted`` of 0 .. N in
    the sorted cells); it then serves every table, every ``reduce_entries`` and every backward of that walk.  Nothing
    here synchronises with the device.  Cells outside 0 .. num_cells-1 raise when ``seg["cells"]`` lives on the CPU; on
    the device the check would be a synchronisation the caller has not asked for, and ``reduce_entries`` skips such
    entries instead."""
    cells = seg["cells"]
    if not isinstance(cells, torch.Tensor) or cells.dim() != 1:
        raise RuntimeError("seg['cells'] must be a tensor [S]")
    if cells.dtype not in (torch.uint32, torch.int32, torch.int64):
        raise RuntimeError("seg['cells'] must have uint32, int32 or int64 dtype")
    if isinstance(num_cells, bool) or not isinstance(num_cells, int) or num_cells < 0:
        raise RuntimeError("num_cells must be a non-negative int")
    cells = cells.to(torch.int64).contiguous()
    if not cells.is_cuda and cells.numel() and (int(cells.min()) < 0 or int(cells.max()) >= num_cells):
        raise RuntimeError("seg['cells'] must lie in 0 .. num_cells-1")
    sorted_cells, entries = torch.sort(cells, stable=True)
    edges = torch.arange(num_cells + 1, dtype=torch.int64, device=cells.device)
    cell_offsets = torch.searchsorted(sorted_cells, edges)       # the number of entries in cells below c
    return CellEntries(num_cells, cells, cell_offsets, entries, sorted_cells)


def _check_index(index):
    if not isinstance(index, CellEntries):
        raise RuntimeError("index must be the CellEntries that cell_entries returns")
    return index.cells.numel()


def _check_values(index, values, what, rows, rows_text):
    if not isinstance(values, torch.Tensor) or values.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f"{what} must have float32 or float64 dtype")
    if values.dim() not in (1, 2) or values.size(0) != rows or (values.dim() == 2 and values.size(1) < 1):
        raise RuntimeError(f"expected {what} {rows_text}")
    if values.device != index.cells.device:
        raise RuntimeError(f"{what} must live on the device of the index")


def _reduce_entries_torch(index, values):
    """The definition: a float64 ``index_add`` over the cell of every entry, cast back.  Autograd differentiates it."""
    out = torch.zeros((index.num_cells,) + values.shape[1:], dtype=torch.float64, device=values.device)
    return out.index_add(0, index.cells, values.to(torch.float64)).to(values.dtype)


def _reduce_entries_hip(index, values):
    """[N] or [N, C] float32 through rf_reduce_entries; ``values`` float32 on the device, not recorded by autograd."""
    from . import _lib
    from .pipeline import _ptr, _stream_ptr

    dev, total = values.device, values.size(0)
    channels = values.size(1) if values.dim() == 2 else 1
    if channels >= 2 ** 31:
        raise RuntimeError("too many channels for the kernel")
    shape = (index.num_cells,) + values.shape[1:]
    if index.num_cells == 0 or total == 0:
        return torch.zeros(shape, dtype=torch.float32, device=dev)
    lib = _lib.load()
    values_c = values.detach().contiguous()
    out = torch.empty(shape, dtype=torch.float32, device=dev)             # cleared, then written, by the library
    ws_bytes = int(lib.rf_reduce_entries_workspace_bytes(total, channels))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.rf_reduce_entries(index.num_cells, total, _ptr(index.sorted_cells), _ptr(index.entries),
                                   _ptr(values_c), channels, _ptr(out), _ptr(ws), ws.numel() * 8, _stream_ptr(dev))
    _lib.check(rc)
    return out


class _ReduceEntries(torch.autograd.Function):
    """``reduce_entries`` through the kernel; the backward is the lookup ``grad[cells]``."""

    @staticmethod
    def forward(ctx, values, index):
        ctx.index = index
        return _reduce_entries_hip(index, values)

    @staticmethod
    def backward(ctx, grad_out):
        return gather_cells(ctx.index, grad_out), None


def reduce_entries(index: CellEntries, values: torch.Tensor, backend=None) -> torch.Tensor:
    """The sum per cell of a per-entry quantity over the walk ``index = cell_entries(seg, N)``:

        out[c] = sum of values[e] over the entries e of cell c

    for ``values`` [S] or [S, C], C >= 1, float32 or float64 on the device of the index; the result is [N] or [N, C]
    with the dtype and device of ``values``, exact zeros for a cell without entries.  With the compositing weights of
    ``composite_entries``' docstring as ``values`` it is ``trace_forward(return_contribution=True)`` for a shading model
    of one's own (examples/cell_statistics.py).  Differentiable in ``values``: the backward is the lookup
    ``grad[cells]``.

    ``backend``: None, "hip" or "torch", as in ``composite_entries``.  None is "hip" for float32 CUDA ``values`` and
    "torch" for everything else.  "hip" runs the kernels of rf_cell_reduce.hip: a wave owns a fixed chunk of the sorted
    positions whatever the cells' list lengths are, sums runs of equal cell in double with the segmented scan of
    rf_ray_sweep.hpp, rounds once to float32; lists that cross chunks are finished in chunk order by a second launch;
    no atomics, every element written once after one clearing fill, the same bits from call to call.  Entries whose
    cell lies outside 0 .. N-1 are skipped.  "torch" is a float64 ``index_add`` over ``index.cells``, cast back."""
    total = _check_index(index)
    _check_values(index, values, "values", total, "[S] or [S, C] with C >= 1, one row per entry of the index")
    if _choose_backend(backend, values, "values") == "torch":
        return _reduce_entries_torch(index, values)
    return _ReduceEntries.apply(values, index)


class _GatherCells(torch.autograd.Function):
    """``table[cells]`` whose backward is ``reduce_entries`` of the incoming gradient."""

    @staticmethod
    def forward(ctx, table, index, backend):
        ctx.index, ctx.backend = index, backend
        return table.index_select(0, index.cells)

    @staticmethod
    def backward(ctx, grad_out):
        backend = ctx.backend
        if backend == "hip" and (not grad_out.is_cuda or grad_out.dtype != torch.float32):
            backend = "torch"                                      # the kernel takes float32 CUDA gradients only
        return reduce_entries(ctx.index, grad_out, backend=backend), None, None


def gather_cells(index: CellEntries, table: torch.Tensor, backend=None) -> torch.Tensor:
    """``table[index.cells]`` for a per-cell ``table`` [N] or [N, C], float32 or float64 on the device of the index: the
    value of every entry's cell, [S] or [S, C].  The forward is torch's ``index_select``.  What this adds is the
    backward: ``reduce_entries(index, grad)`` instead of torch's scatter-add, so that

        sigma = radfoam.gather_cells(index, softplus(density))

    is the deterministic spelling of ``softplus(density)[cells]``: the gradient of the table is summed in double
    through the index built once per walk, without atomics, the same bits from call to call.

    ``backend`` chooses how the backward sums, as in ``reduce_entries``: None or "hip" run the kernel for float32 CUDA
    gradients and the float64 ``index_add`` for everything else; "torch" always the latter.  "hip" takes a float32 CUDA
    ``table``.  As for ``table[cells]``, every cell of the walk must lie in 0 .. N-1."""
    _check_index(index)
    _check_values(index, table, "table", index.num_cells, "[N] or [N, C] with C >= 1, one row per cell of the index")
    chosen = _choose_backend(backend, table, "table")
    if index.cells.numel() and index.num_cells == 0:
        raise RuntimeError("an index with entries needs cells to look up")
    return _GatherCells.apply(table, index, chosen)
