"""The tracer's own shading model per ENTRY of an exported walk (``Pipeline.trace_segments``): a per-cell table of
spherical-harmonic coefficients evaluated in the direction of the entry's ray.

``sh_entries`` is the one colour model the walk operators could not express without materialising ``coeffs[cells]``
([S, 3K]) and a gradient of that size.  For float32 tensors on the device it runs the kernels of rf_sh_entries.hip: the
forward gives the tracer's colour bit for bit, the gradient of the table is the deterministic sum per cell of
``reduce_entries`` with the row formed in registers, the gradient of the directions a segmented sum per ray.  Everything
else is a plain torch restatement differentiated by autograd.
"""
from __future__ import annotations

import torch

from .cells import CellEntries, _check_index
from .segments import _check_offsets, _choose_backend, _entry_rays

_WIDTHS = {3: 0, 12: 1, 27: 2, 48: 3}


def _sh_basis(d, degree):
    """[R, K]: the basis of oracle sh_basis / rf_math.hpp sh_basis<DEG> at the unit vectors ``d`` [R, 3], the
    polynomials as written there."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    c1 = 0.4886025119029199
    sh = [0.0 * x + 0.28209479177387814]                             # constant; its direction gradient zeros, not None
    if degree > 0:
        sh += [-c1 * y, c1 * z, -c1 * x]
    if degree > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        sh += [1.0925484305920792 * xy, -1.0925484305920792 * yz, 0.31539156525252005 * ((2.0 * zz - xx) - yy),
               -1.0925484305920792 * xz, 0.5462742152960396 * (xx - yy)]
        if degree > 2:
            sh += [(-0.5900435899266435 * y) * (3.0 * xx - yy), (2.890611442640554 * xy) * z,
                   (-0.4570457994644658 * y) * ((4.0 * zz - xx) - yy),
                   (0.3731763325901154 * z) * ((2.0 * zz - 3.0 * xx) - 3.0 * yy),
                   (-0.4570457994644658 * x) * ((4.0 * zz - xx) - yy), (1.445305721320277 * z) * (xx - yy),
                   (-0.5900435899266435 * x) * (xx - 3.0 * yy)]
    return torch.stack(sh, dim=-1)


def _sh_entries_torch(offsets, index, coeffs, directions, degree):
    """The definition, in the dtype of ``coeffs``.  Autograd differentiates it; ``where`` gives the clamp the
    reference's gradient: zero where the colour is zero."""
    d = directions.reshape(-1, 3).to(coeffs.dtype)
    d = d / d.square().sum(dim=-1, keepdim=True).sqrt()
    basis = _sh_basis(d, degree)                                                     # [R, K]
    ray = _entry_rays(offsets, index.cells.numel())
    rows = coeffs.index_select(0, index.cells).reshape(-1, basis.size(1), 3)         # [S, K, 3]
    pre = 0.5 + (basis.index_select(0, ray).unsqueeze(-1) * rows).sum(dim=1)
    return torch.where(pre > 0, pre, torch.zeros_like(pre))


class _ShEntries(torch.autograd.Function):
    """``sh_entries`` through the kernels of rf_sh_entries.hip: float32 CUDA ``coeffs``.  Kept for the backward: the
    colour (its zeros are the clamp's mask), the ray of every entry, the index and the offsets."""

    @staticmethod
    def forward(ctx, coeffs, directions, index, offsets, degree):
        from . import _lib
        from .pipeline import _ptr, _stream_ptr

        dev, total, num_rays = coeffs.device, index.cells.numel(), offsets.numel() - 1
        if num_rays >= 2 ** 31:
            raise RuntimeError("too many rays for the kernel")
        width = coeffs.size(1)
        table = coeffs.detach()
        if table.stride(1) != 1 or (table.size(0) > 1 and table.stride(0) < width) or table.stride(0) >= 2 ** 31:
            table = table.contiguous()                           # a column slice of the attributes is read in place
        pitch = table.stride(0) if table.size(0) > 1 else width
        dirs = directions.detach().reshape(-1, 3).to(torch.float32).contiguous()
        entry_rays = _entry_rays(offsets, total, dtype=torch.int32)      # built once, kept for the backward
        rgb = torch.empty((total, 3), dtype=torch.float32, device=dev)   # every element is written
        if total > 0:
            with torch.cuda.device(dev):
                rc = _lib.load().rf_sh_entries_forward(degree, index.num_cells, total, num_rays, _ptr(index.cells),
                                                       _ptr(entry_rays), _ptr(table), pitch, _ptr(dirs), _ptr(rgb),
                                                       _stream_ptr(dev))
            _lib.check(rc)
        ctx.index, ctx.degree, ctx.pitch = index, degree, pitch
        ctx.directions = (directions.dtype, directions.shape)
        ctx.save_for_backward(rgb, entry_rays, offsets, table, dirs)
        return rgb

    @staticmethod
    def backward(ctx, grad_out):
        from . import _lib
        from .pipeline import _ptr, _stream_ptr

        rgb, entry_rays, offsets, table, dirs = ctx.saved_tensors
        index, degree = ctx.index, ctx.degree
        dev, total, num_rays, num_cells = rgb.device, rgb.size(0), offsets.numel() - 1, index.num_cells
        width = 3 * (degree + 1) ** 2
        lib = _lib.load()
        grad = grad_out.to(torch.float32).contiguous()
        grad_coeffs = grad_directions = None
        if ctx.needs_input_grad[0]:
            grad_coeffs = torch.empty((num_cells, width), dtype=torch.float32, device=dev)   # cleared by the library
            ws_bytes = int(lib.rf_sh_entries_workspace_bytes(total, degree))
            ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.float64, device=dev)
            with torch.cuda.device(dev):
                rc = lib.rf_sh_entries_backward_coeffs(degree, num_cells, total, num_rays, _ptr(index.sorted_cells),
                                                       _ptr(index.entries), _ptr(entry_rays), _ptr(dirs), _ptr(rgb),
                                                       _ptr(grad), _ptr(grad_coeffs), _ptr(ws), ws.numel() * 8,
                                                       _stream_ptr(dev))
            _lib.check(rc)
        if ctx.needs_input_grad[1]:
            dtype, shape = ctx.directions
            if degree == 0 or total == 0 or num_rays == 0 or num_cells == 0:
                grad_directions = torch.zeros(shape, dtype=dtype, device=dev)        # a constant colour: no launch
            else:
                out = torch.empty((num_rays, 3), dtype=torch.float32, device=dev)    # every element is written
                with torch.cuda.device(dev):
                    rc = lib.rf_sh_entries_backward_directions(degree, num_cells, total, num_rays, _ptr(offsets),
                                                               _ptr(index.cells), _ptr(table), ctx.pitch, _ptr(dirs),
                                                               _ptr(rgb), _ptr(grad), _ptr(out), _stream_ptr(dev))
                _lib.check(rc)
                grad_directions = out.to(dtype).reshape(shape)
        return grad_coeffs, grad_directions, None, None, None


def sh_entries(seg, index: CellEntries, coeffs: torch.Tensor, directions: torch.Tensor, backend=None) -> torch.Tensor:
    """rgb [S, 3]: the tracer's spherical-harmonic colour of every entry of the walk ``seg`` (the dict
    ``Pipeline.trace_segments`` or ``trace_differentiable_segments`` returns; only ``offsets``, int64 [R+1], is read)
    with ``index = cell_entries(seg, N)``, for a per-cell table ``coeffs`` [N, 3K], K = (D+1)^2, D = 0 .. 3 taken from
    the width, in the layout of ``attributes[:, :-1]`` (element i is channel i % 3 of basis function i // 3), and the rays'
    ``directions`` [R, 3] (any leading shape that flattens to R, such as ``rays[..., 3:6]``; neither unit length nor
    contiguous is asked for).  Per entry e of ray r in cell n:

        dhat = d_r / |d_r|,      rgb[e, c] = max(0.5 + sum_k Y_k(dhat) coeffs[n, 3k + c], 0)

    with the basis Y of the tracer (rf_math.hpp ``sh_basis``).  The result has the dtype of ``coeffs``.  The tracer's
    density gate is NOT part of it: ``trace_forward`` gives colour 0 to cells of density <= 1e-6, which is one line,

        rgb = rgb * (radfoam.gather_cells(index, density) > 1e-6).unsqueeze(-1)

    so that ``composite_entries(seg, gather_cells(index, density), rgb)`` reproduces ``trace_forward`` at every degree
    (examples/sh_shading.py), and each of its parts can be replaced.

    Differentiable in ``coeffs`` and in ``directions``.  The gradient of the clamp is zero where rgb == 0 (the
    reference's rule).  The gradient of the directions goes through the polynomials and then through the
    normalisation, ``(q - dhat (dhat . q)) / |d|``; at D = 0 it is exact zeros.  Gradients come back in the shape and
    dtype of the caller's tensors.

    ``backend``: None, "hip" or "torch", as in ``composite_entries``.  None is "hip" for float32 CUDA ``coeffs`` and
    "torch" for everything else.  "hip" runs the kernels of rf_sh_entries.hip: the forward is the tracer's colour BIT
    FOR BIT (its normalisation, basis and chain of fused multiply-adds), one lane per entry, and never forms
    ``coeffs[cells]``; the gradient of ``coeffs`` is summed per cell in double through the index, rounded once, without
    atomics; the gradient of ``directions`` is summed per ray in double.  Two calls give the same bits, gradients
    included.  Entries whose cell lies outside 0 .. N-1 get zeros.  "torch" is the definition above in plain torch, in
    the dtype of ``coeffs``, differentiated by autograd."""
    total = _check_index(index)
    if not isinstance(coeffs, torch.Tensor) or coeffs.dtype not in (torch.float16, torch.float32, torch.float64):
        raise RuntimeError("coeffs must have float16, float32 or float64 dtype")
    if coeffs.dim() != 2 or coeffs.size(0) != index.num_cells or coeffs.size(1) not in _WIDTHS:
        raise RuntimeError("expected coeffs [N, 3K] with K = 1, 4, 9 or 16 (SH degree 0 .. 3), one row per cell of the "
                           "index")
    if not isinstance(directions, torch.Tensor) or not directions.is_floating_point():
        raise RuntimeError("directions must be a floating-point tensor")
    offsets = seg["offsets"]
    if not isinstance(offsets, torch.Tensor):
        raise RuntimeError("seg['offsets'] must be int64 [R+1]")
    num_rays = _check_offsets(offsets).numel() - 1
    if directions.dim() < 1 or directions.size(-1) != 3 or directions.numel() != 3 * num_rays:
        raise RuntimeError("expected directions [R, 3] (any leading shape of R rays), one row per ray of "
                           "seg['offsets']")
    dev = coeffs.device
    if index.cells.device != dev or directions.device != dev or offsets.device != dev:
        raise RuntimeError("the index, directions and seg['offsets'] must live on the device of coeffs")
    if total and index.num_cells == 0:
        raise RuntimeError("an index with entries needs cells to look up")
    if not offsets.is_cuda and int(offsets[-1]) != total:
        raise RuntimeError("seg['offsets'][-1] must be the number of entries of the index")
    degree = _WIDTHS[coeffs.size(1)]
    if _choose_backend(backend, coeffs, "coeffs") == "torch":
        return _sh_entries_torch(offsets, index, coeffs, directions, degree)
    return _ShEntries.apply(coeffs, directions, index, offsets.contiguous(), degree)
