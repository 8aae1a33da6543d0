"""Compositing over an exported walk (``Pipeline.trace_segments``) in plain torch, so that a caller's own shading model --
any per-cell density and colour it can compute with autograd -- is rendered along the very intervals the tracer uses.

No kernel of its own: a handful of elementwise operations, one cumulative sum and two scatter-adds over the [S] entries.
"""
from __future__ import annotations

import torch


def composite_segments(seg, density: torch.Tensor, rgb: torch.Tensor) -> torch.Tensor:
    """rgba [R, 4] of the rays of ``seg`` (the dict ``Pipeline.trace_segments`` returns: ``offsets`` int64 [R+1],
    ``cells`` [S], ``t_enter`` / ``t_exit`` float32 [S]) for a per-cell ``density`` [N] and ``rgb`` [N, 3]:

        dt = max(t_exit - t_enter, 0), 0 where t_exit is infinite (the cell the walk ends in has no far side)
        alpha = 1 - exp(-density[cell] dt),  T = prod of (1 - alpha) over the ray's earlier entries,  w = T alpha
        rgb_out = sum of w rgb[cell],  alpha_out = 1 - prod of (1 - alpha) over all of the ray's entries

    which is the compositing of ``trace_forward`` with the colour model left to the caller (trace_forward's own is
    ``max(0.5 + SH . coefficients, 0)``, and 0 for cells of density <= 1e-6).  Differentiable in ``density`` and
    ``rgb``; float32 or float64, on any device (the entries of ``seg`` are moved to the device of ``density``).  The
    result has the dtype of ``density``.

    Vectorised over the CSR: log(1 - alpha) is -density dt exactly, so the transmittance in front of every entry is the
    exponential of a segmented exclusive cumulative sum.  That sum runs over all S entries at once and the ray's own
    part is a difference of two of its values, so it is formed in float64 whatever the dtype of the inputs.  No Python
    loop over rays and no synchronisation with the device."""
    if density.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("density must have float32 or float64 dtype")
    if rgb.dtype != density.dtype or rgb.device != density.device:
        raise RuntimeError("rgb must have the dtype and device of density")
    if density.dim() != 1 or rgb.dim() != 2 or rgb.size(-1) != 3 or rgb.size(0) != density.size(0):
        raise RuntimeError("expected density [N] and rgb [N, 3]")
    dev, dtype = density.device, density.dtype
    offsets = seg["offsets"].to(dev)
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 1:
        raise RuntimeError("seg['offsets'] must be int64 [R+1]")
    cells = seg["cells"].to(dev).to(torch.int64)
    num_rays, total = offsets.numel() - 1, cells.numel()
    if seg["t_enter"].numel() != total or seg["t_exit"].numel() != total:
        raise RuntimeError("seg['cells'], seg['t_enter'] and seg['t_exit'] must have one element per entry")
    t_enter = seg["t_enter"].to(dev).to(torch.float64)
    t_exit = seg["t_exit"].to(dev).to(torch.float64)
    dt = torch.where(torch.isinf(t_exit), torch.zeros_like(t_exit), (t_exit - t_enter).clamp_min(0.0))

    log_keep = -density[cells].to(torch.float64) * dt              # log(1 - alpha) of every entry
    run = torch.cumsum(log_keep, 0)                                # inclusive, across ray boundaries
    run0 = torch.cat([run.new_zeros(1), run])                      # run0[e] = sum of the entries before e
    counts = offsets[1:] - offsets[:-1]
    ray = torch.repeat_interleave(torch.arange(num_rays, device=dev), counts, output_size=total)
    before = run0[offsets[:-1]]                                    # [R]: the sum in front of each ray's first entry
    transmittance = torch.exp(run0[:-1] - before[ray])             # in front of every entry, within its ray
    weight = transmittance * -torch.expm1(log_keep)

    out = torch.zeros((num_rays, 4), dtype=torch.float64, device=dev)
    colour = out[:, :3].index_add(0, ray, weight.unsqueeze(-1) * rgb[cells].to(torch.float64))
    alpha = -torch.expm1(run0[offsets[1:]] - before)
    return torch.cat([colour, alpha.unsqueeze(-1)], dim=-1).to(dtype)
