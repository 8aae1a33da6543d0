"""Compositing over an exported walk (``Pipeline.trace_segments``) in plain torch, so that a caller's own shading model --
any per-cell density and colour it can compute with autograd -- is rendered along the very intervals the tracer uses.

``composite_segments`` has no kernel of its own: a handful of elementwise operations, one cumulative sum and two
scatter-adds over the [S] entries.  It reads ``t_enter`` / ``t_exit`` with ordinary torch operations, so when those two
carry a ``grad_fn`` with respect to the points or the rays (``Pipeline.trace_differentiable_segments``) everything
composited from them is differentiable in the geometry and in the camera.  The backward operators behind that are
``segment_points_grad`` and ``segment_rays_grad``: HIP kernels (rf_segments_grad.hip, rf_segments_rays_grad.hip) on the
device, vectorised torch restatements of the same definitions elsewhere.

``composite_entries`` is the same compositing for inputs the caller has per ENTRY (a density [S] and any number of
channels [S, C]), with kernels of its own for float32 tensors on the device (rf_composite.hip).
``ray_distortion`` is the regulariser that goes with it: Mip-NeRF 360's distortion loss of every ray from the same
per-entry density, by the same scheme of kernels (rf_distortion.hip).  ``ray_quantiles`` is the depth
output: where along the ray the transmittance of that density falls through given levels (rf_quantiles.hip, DESIGN
4.14).  ``entry_weights`` gives the compositing weight and the transmittance of every entry themselves, for whatever is
not a sum of them along the ray (rf_entry_weights.hip).
"""
from __future__ import annotations

import torch

from . import _lib
from .scene_ops import _ptr, _stream


def _check_offsets(offsets):
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 1:
        raise RuntimeError("seg['offsets'] must be int64 [R+1]")
    return offsets


def _choose_backend(backend, tensor, what, any_dtype=False):
    """"hip" or "torch" from ``backend`` None, "hip" or "torch".  None is "hip" for a float32 CUDA ``tensor`` (for every
    CUDA ``tensor`` with ``any_dtype``) and "torch" for everything else; "hip" takes a float32 CUDA ``tensor``."""
    if backend not in (None, "hip", "torch"):
        raise ValueError("backend must be None, 'hip' or 'torch'")
    if backend is None:
        backend = "hip" if tensor.is_cuda and (any_dtype or tensor.dtype == torch.float32) else "torch"
    if backend == "hip" and (not tensor.is_cuda or tensor.dtype != torch.float32):
        raise RuntimeError(f"the kernel takes float32 CUDA {what} (backend='torch' restates it for anything else)")
    return backend


def _entry_rays(offsets, total, dtype=torch.int64):
    """[S]: the ray of every entry, on the device of ``offsets``."""
    rays = torch.arange(offsets.numel() - 1, dtype=dtype, device=offsets.device)
    return torch.repeat_interleave(rays, offsets[1:] - offsets[:-1], output_size=total)


def _sums_in_ray(v, offsets, ray):
    """The sum of ``v`` [S] over the ray's earlier entries [S], and over all of each ray's entries [R]: differences of
    one cumulative sum over the whole list."""
    run0 = torch.cat([v.new_zeros(1), torch.cumsum(v, 0)])         # run0[e] = sum of the entries before e
    first = run0[offsets[:-1]]                                     # [R]: the sum in front of each ray's first entry
    return run0[:-1] - first[ray], run0[offsets[1:]] - first


def _times_for_kernel(ctx, dev, t_enter, t_exit):
    """The times as the kernels read them (float32 [S] on ``dev``); ``ctx`` records what their gradients must match."""
    ctx.times = tuple((t.dtype, t.device, t.shape) for t in (t_enter, t_exit))
    return tuple(t.detach().to(dev).to(torch.float32).reshape(-1).contiguous() for t in (t_enter, t_exit))


def _times_grads(ctx, grad_t_enter, grad_t_exit):
    """The kernels' gradients of the times in the dtype, device and shape the caller's times had."""
    return tuple(None if g is None else g.to(device).to(dtype).reshape(shape)
                 for g, (dtype, device, shape) in zip((grad_t_enter, grad_t_exit), ctx.times))


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
    dev = density.device
    offsets = _check_offsets(seg["offsets"].to(dev))
    cells = seg["cells"].to(dev).to(torch.int64)
    total = cells.numel()
    if seg["t_enter"].numel() != total or seg["t_exit"].numel() != total:
        raise RuntimeError("seg['cells'], seg['t_enter'] and seg['t_exit'] must have one element per entry")
    return _composite_entries_torch(offsets, seg["t_enter"], seg["t_exit"], density[cells], rgb[cells])


def _check_entries_inputs(seg, sigma, values):
    if sigma.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("sigma must have float32 or float64 dtype")
    if values.dtype != sigma.dtype or values.device != sigma.device:
        raise RuntimeError("values must have the dtype and device of sigma")
    if sigma.dim() != 1 or values.dim() != 2 or values.size(-1) < 1:
        raise RuntimeError("expected sigma [S] and values [S, C] with C >= 1")
    offsets = _check_offsets(seg["offsets"])
    total = sigma.size(0)
    if seg["t_enter"].numel() != total or seg["t_exit"].numel() != total or values.size(0) != total:
        raise RuntimeError("sigma, values, seg['t_enter'] and seg['t_exit'] must have one element (row) per entry")
    return offsets.numel() - 1, total


def _composite_entries_torch(offsets, t_enter, t_exit, sigma, values):
    """The definition, and ``composite_segments``: float64 throughout, a segmented exclusive cumulative sum for the
    transmittance, one ``index_add`` over the ray index.  Autograd differentiates it.  ``offsets`` is on the device of
    ``sigma``."""
    dev, dtype = sigma.device, sigma.dtype
    num_rays, total = offsets.numel() - 1, sigma.size(0)
    t_enter = t_enter.to(dev).to(torch.float64).reshape(-1)
    t_exit = t_exit.to(dev).to(torch.float64).reshape(-1)
    dt = torch.where(torch.isinf(t_exit), torch.zeros_like(t_exit), (t_exit - t_enter).clamp_min(0.0))

    log_keep = -sigma.to(torch.float64) * dt                       # -x = log(1 - alpha) of every entry
    ray = _entry_rays(offsets, total)
    log_before, log_ray = _sums_in_ray(log_keep, offsets, ray)
    transmittance = torch.exp(log_before)                          # in front of every entry, within its ray
    weight = transmittance * -torch.expm1(log_keep)

    out = torch.zeros((num_rays, values.size(1)), dtype=torch.float64, device=dev)
    composited = out.index_add(0, ray, weight.unsqueeze(-1) * values.to(torch.float64))
    alpha = -torch.expm1(log_ray)
    return torch.cat([composited, alpha.unsqueeze(-1)], dim=-1).to(dtype)


class _CompositeEntries(torch.autograd.Function):
    """``composite_entries`` through the kernels of rf_composite.hip: float32 CUDA tensors, each gradient only where
    its input needs one.  Nothing but the inputs is kept for the backward, which sweeps the list again."""

    @staticmethod
    def forward(ctx, sigma, values, t_enter, t_exit, offsets):

        dev = sigma.device
        num_rays, total, channels = offsets.numel() - 1, sigma.size(0), values.size(1)
        if num_rays >= 2 ** 31 or channels >= 2 ** 31:
            raise RuntimeError("too many rays or channels for the kernel")
        offsets = offsets.to(dev).contiguous()
        sigma_c, values_c = sigma.detach().contiguous(), values.detach().contiguous()
        t_enter_c, t_exit_c = _times_for_kernel(ctx, dev, t_enter, t_exit)
        ctx.save_for_backward(sigma_c, values_c, t_enter_c, t_exit_c, offsets)
        if num_rays == 0 or total == 0:
            return torch.zeros((num_rays, channels + 1), dtype=torch.float32, device=dev)
        out = torch.empty((num_rays, channels + 1), dtype=torch.float32, device=dev)     # every element is written
        with torch.cuda.device(dev):
            rc = _lib.load().rf_composite_entries_forward(
                num_rays, _ptr(offsets), total, _ptr(t_enter_c), _ptr(t_exit_c), _ptr(sigma_c), _ptr(values_c),
                channels, _ptr(out), _stream(dev))
        _lib.check(rc)
        return out

    @staticmethod
    def backward(ctx, grad_out):

        sigma, values, t_enter, t_exit, offsets = ctx.saved_tensors
        dev = sigma.device
        num_rays, total, channels = offsets.numel() - 1, sigma.size(0), values.size(1)
        want = ctx.needs_input_grad[:4]
        # entries outside offsets[0] .. offsets[R] are not written by the kernel: there are none in a sound list
        grads = [torch.empty_like(t) if w else None for t, w in zip((sigma, values, t_enter, t_exit), want)]
        if num_rays > 0 and total > 0 and any(want):
            grad_out = grad_out.to(torch.float32).contiguous()
            with torch.cuda.device(dev):
                rc = _lib.load().rf_composite_entries_backward(
                    num_rays, _ptr(offsets), total, _ptr(t_enter), _ptr(t_exit), _ptr(sigma), _ptr(values), channels,
                    _ptr(grad_out), _ptr(grads[0]), _ptr(grads[1]), _ptr(grads[2]), _ptr(grads[3]), _stream(dev))
            _lib.check(rc)
        return (grads[0], grads[1], *_times_grads(ctx, grads[2], grads[3]), None)


def composite_entries(seg, sigma: torch.Tensor, values: torch.Tensor, backend=None) -> torch.Tensor:
    """[R, C+1] for the rays of ``seg`` (the dict ``Pipeline.trace_segments`` or ``trace_differentiable_segments``
    returns; ``offsets`` int64 [R+1] and ``t_enter`` / ``t_exit`` [S] are read, ``cells`` is not) from values the caller
    has PER ENTRY: ``sigma`` [S] and ``values`` [S, C], C >= 1, of one dtype (float32 or float64) and device.  Per ray,
    over its entries in order (the compositing of ``composite_segments``):

        dt = 0 where t_exit is infinite, else max(t_exit - t_enter, 0),      x = sigma dt
        T = exp(-(sum of x over the ray's earlier entries)),      w = T (1 - exp(-x))
        out[r, c] = sum of w values[:, c],      out[r, C] = 1 - exp(-(sum of x))

    Channels 0 .. C-1 are the composited values, channel C is the opacity; a ray without entries gives a row of zeros;
    the result has the dtype of ``sigma``.  ``composite_entries(seg, density[cells], rgb[cells])`` is
    ``composite_segments(seg, density, rgb)``; what this adds is everything a per-cell table cannot hold: a colour that
    depends on the ray (examples/view_dependent_shading.py), more than three channels, a density of the entry.

    Differentiable in ``sigma``, ``values``, ``seg["t_enter"]`` and ``seg["t_exit"]`` (which carry the gradient on to
    the points and the rays when they come from ``trace_differentiable_segments``).  The times' gradient follows
    torch's ``clamp_min``: an entry with t_exit >= t_enter, both finite, passes it on, t_exit < t_enter does not, and
    an entry with an infinite t_exit gets exact zeros in every gradient.

    ``backend``: None, "hip" or "torch".  None is "hip" for float32 CUDA ``sigma`` and "torch" for everything else.
    "hip" runs the kernels of rf_composite.hip (one wave owns a run of consecutive rays, sums in double, one rounding
    to float32, no atomics: the same bits from call to call, gradients included; the times are read as float32).
    "torch" is a vectorised restatement with ``composite_segments``' float64 segmented cumulative sum, differentiated by
    autograd, on any device; no Python loop over rays.  ``offsets[-1] == S`` is checked on the torch path only, and
    there only when ``seg["offsets"]`` lives on the CPU: on the device the check would be a synchronisation the caller
    has not asked for.  (The kernels clamp every offset to 0 .. S instead.)"""
    num_rays, total = _check_entries_inputs(seg, sigma, values)
    if _choose_backend(backend, sigma, "sigma and values") == "torch":
        if not seg["offsets"].is_cuda and int(seg["offsets"][-1]) != total:
            raise RuntimeError("seg['offsets'][-1] must be the number of entries")
        return _composite_entries_torch(seg["offsets"].to(sigma.device), seg["t_enter"], seg["t_exit"], sigma, values)
    return _CompositeEntries.apply(sigma, values, seg["t_enter"], seg["t_exit"], seg["offsets"])


def _check_distortion_inputs(seg, sigma, s_enter, s_exit):
    if sigma.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("sigma must have float32 or float64 dtype")
    if (s_enter is None) != (s_exit is None):
        raise RuntimeError("s_enter and s_exit must both be given or both be omitted")
    for s in (s_enter, s_exit):
        if s is not None and (s.dtype != sigma.dtype or s.device != sigma.device):
            raise RuntimeError("s_enter and s_exit must have the dtype and device of sigma")
    if sigma.dim() != 1 or (s_enter is not None and (s_enter.dim() != 1 or s_exit.dim() != 1)):
        raise RuntimeError("expected sigma [S], and s_enter [S] and s_exit [S] where given")
    offsets = _check_offsets(seg["offsets"])
    total = sigma.size(0)
    if seg["t_enter"].numel() != total or seg["t_exit"].numel() != total or (
            s_enter is not None and (s_enter.size(0) != total or s_exit.size(0) != total)):
        raise RuntimeError("sigma, s_enter, s_exit, seg['t_enter'] and seg['t_exit'] must have one element per entry")
    return offsets.numel() - 1, total


def _ray_distortion_torch(offsets, t_enter, t_exit, sigma, s_enter, s_exit):
    """The definition with the operations of ``_composite_entries_torch``: float64 throughout, the sums over a ray's
    earlier entries as differences of list-wide cumulative sums, one ``index_add`` over the ray index.  Autograd
    differentiates it."""
    dev, dtype = sigma.device, sigma.dtype
    num_rays, total = offsets.numel() - 1, sigma.size(0)
    t_enter = t_enter.to(dev).to(torch.float64).reshape(-1)
    t_exit = t_exit.to(dev).to(torch.float64).reshape(-1)
    infinite, zero = torch.isinf(t_exit), torch.zeros_like(t_exit)
    dt = torch.where(infinite, zero, (t_exit - t_enter).clamp_min(0.0))
    a, b = (t_enter, t_exit) if s_enter is None else (s_enter.to(torch.float64), s_exit.to(torch.float64))
    mid = torch.where(infinite, zero, (a + b) / 2)                 # selected: no inf * 0, and no gradient either
    width = torch.where(infinite, zero, (b - a).clamp_min(0.0))

    x = sigma.to(torch.float64) * dt
    ray = _entry_rays(offsets, total)

    def before(v):                                                 # the sum of v over the ray's earlier entries
        return _sums_in_ray(v, offsets, ray)[0]

    weight = torch.exp(-before(x)) * -torch.expm1(-x)
    per_entry = 2 * weight * (mid * before(weight) - before(weight * mid)) + weight * weight * width / 3
    return torch.zeros(num_rays, dtype=torch.float64, device=dev).index_add(0, ray, per_entry).to(dtype)


class _RayDistortion(torch.autograd.Function):
    """``ray_distortion`` through the kernels of rf_distortion.hip: float32 CUDA tensors, each gradient only where its
    input needs one.  Nothing but the inputs is kept for the backward, which sweeps the list twice."""

    @staticmethod
    def forward(ctx, sigma, t_enter, t_exit, s_enter, s_exit, offsets):

        dev = sigma.device
        num_rays, total = offsets.numel() - 1, sigma.size(0)
        if num_rays >= 2 ** 31:
            raise RuntimeError("too many rays for the kernel")
        offsets = offsets.to(dev).contiguous()
        sigma_c = sigma.detach().contiguous()
        t_enter_c, t_exit_c = _times_for_kernel(ctx, dev, t_enter, t_exit)
        ctx.own_measure = s_enter is not None
        saved = [sigma_c, t_enter_c, t_exit_c, offsets]
        if ctx.own_measure:
            saved += [s_enter.detach().contiguous(), s_exit.detach().contiguous()]
        ctx.save_for_backward(*saved)
        if num_rays == 0 or total == 0:
            return torch.zeros(num_rays, dtype=torch.float32, device=dev)
        out = torch.empty(num_rays, dtype=torch.float32, device=dev)                     # every element is written
        measure = saved[4:] if ctx.own_measure else (None, None)
        with torch.cuda.device(dev):
            rc = _lib.load().rf_ray_distortion_forward(
                num_rays, _ptr(offsets), total, _ptr(t_enter_c), _ptr(t_exit_c), _ptr(sigma_c), _ptr(measure[0]),
                _ptr(measure[1]), _ptr(out), _stream(dev))
        _lib.check(rc)
        return out

    @staticmethod
    def backward(ctx, grad_out):

        sigma, t_enter, t_exit, offsets = ctx.saved_tensors[:4]
        measure = ctx.saved_tensors[4:] if ctx.own_measure else (None, None)
        dev = sigma.device
        num_rays, total = offsets.numel() - 1, sigma.size(0)
        want = ctx.needs_input_grad[:5]
        # entries outside offsets[0] .. offsets[R] are not written by the kernel: there are none in a sound list
        grads = [torch.empty_like(sigma) if w else None for w in want]
        if num_rays > 0 and total > 0 and any(want):
            grad_out = grad_out.to(torch.float32).contiguous()
            with torch.cuda.device(dev):
                rc = _lib.load().rf_ray_distortion_backward(
                    num_rays, _ptr(offsets), total, _ptr(t_enter), _ptr(t_exit), _ptr(sigma), _ptr(measure[0]),
                    _ptr(measure[1]), _ptr(grad_out), _ptr(grads[0]), _ptr(grads[1]), _ptr(grads[2]), _ptr(grads[3]),
                    _ptr(grads[4]), _stream(dev))
            _lib.check(rc)
        return (grads[0], *_times_grads(ctx, grads[1], grads[2]), grads[3], grads[4], None)


def ray_distortion(seg, sigma: torch.Tensor, s_enter=None, s_exit=None, backend=None) -> torch.Tensor:
    """[R]: the distortion regulariser of Mip-NeRF 360 for the rays of ``seg`` (the dict ``Pipeline.trace_segments`` or
    ``trace_differentiable_segments`` returns; ``offsets`` int64 [R+1] and ``t_enter`` / ``t_exit`` [S] are read,
    ``cells`` is not) with a density ``sigma`` [S] PER ENTRY, float32 or float64.  It is small where a ray's compositing
    weights sit close together in depth; ``lambda * ray_distortion(...).mean()`` added to a photometric loss removes
    floaters (examples/distortion_regulariser.py).  Per ray, over its entries i in order (the weights are
    those of ``composite_entries``):

        dt = 0 where t_exit is infinite, else max(t_exit - t_enter, 0),      x = sigma dt
        T_i = exp(-(sum of x_k, k < i)),      w_i = T_i (1 - exp(-x_i))
        a, b = s_enter, s_exit if given, else t_enter, t_exit;      m = (a + b) / 2,      d = max(b - a, 0)
        out[r] = 2 sum_i w_i (m_i W<_i - M<_i) + (1/3) sum_i w_i^2 d_i,   W<_i = sum_{k<i} w_k,  M<_i = sum_{k<i} w_k m_k

    This ordered form is the definition.  It equals ``sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 d_i`` wherever the
    midpoints of the entries that carry weight do not decrease along the ray, which holds for a walk.

    ``s_enter`` / ``s_exit`` ([S], dtype and device of ``sigma``; both or neither) measure the distortion in another
    distance -- normalised, or contracted as s = t / (1 + t) -- while the weights still come from the true t.  THEY MUST
    BE AN INCREASING FUNCTION OF t: otherwise the midpoints are out of order and the ordered form is no longer the
    distortion.  An entry with an infinite ``t_exit`` has w = 0, contributes nothing and gets exact zeros in every
    gradient whatever its ``s_*`` hold; a ray without entries gives 0; a non-finite ``s_*`` at an entry that carries
    weight gives non-finite numbers.  The result has the dtype of ``sigma``.

    Differentiable in ``sigma``, ``seg["t_enter"]`` and ``seg["t_exit"]`` (which carry the gradient on to the points and
    the rays when they come from ``trace_differentiable_segments``), and in ``s_enter`` / ``s_exit`` when given: the
    times then get only the gradient through w, otherwise also the one through m and d.  Both ``max`` follow torch's
    ``clamp_min``: equality passes the gradient on.

    ``backend``: None, "hip" or "torch", as in ``composite_entries``.  None is "hip" for float32 CUDA ``sigma`` and
    "torch" for everything else.  "hip" runs the kernels of rf_distortion.hip (one wave owns a run of consecutive rays,
    segmented scans in double, one rounding to float32, no atomics: the same bits from call to call, gradients
    included; the times are read as float32).  "torch" restates the definition in float64 with list-wide cumulative
    sums, differentiated by autograd, on any device; no Python loop over rays.  ``offsets[-1] == S`` is checked on the
    torch path only, and there only when ``seg["offsets"]`` lives on the CPU.  (The kernels clamp every offset to
    0 .. S instead.)"""
    num_rays, total = _check_distortion_inputs(seg, sigma, s_enter, s_exit)
    if _choose_backend(backend, sigma, "sigma") == "torch":
        if not seg["offsets"].is_cuda and int(seg["offsets"][-1]) != total:
            raise RuntimeError("seg['offsets'][-1] must be the number of entries")
        return _ray_distortion_torch(seg["offsets"].to(sigma.device), seg["t_enter"], seg["t_exit"], sigma, s_enter,
                                     s_exit)
    return _RayDistortion.apply(sigma, seg["t_enter"], seg["t_exit"], s_enter, s_exit, seg["offsets"])


def _check_quantiles_inputs(seg, sigma, quantiles):
    if sigma.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("sigma must have float32 or float64 dtype")
    if quantiles.dtype != sigma.dtype or quantiles.device != sigma.device:
        raise RuntimeError("quantiles must have the dtype and device of sigma")
    if sigma.dim() != 1 or quantiles.dim() < 1 or quantiles.size(-1) < 1:
        raise RuntimeError("expected sigma [S] and quantiles [R, Q] with Q >= 1")
    offsets = _check_offsets(seg["offsets"])
    num_rays, total, num_q = offsets.numel() - 1, sigma.size(0), quantiles.size(-1)
    if seg["t_enter"].numel() != total or seg["t_exit"].numel() != total:
        raise RuntimeError("sigma, seg['t_enter'] and seg['t_exit'] must have one element per entry")
    if quantiles.numel() != num_rays * num_q:
        raise RuntimeError("quantiles must have one row of Q per ray")
    return num_rays, total, num_q


def _quantile_levels(quantiles, num_rays, num_q):
    """[R, Q] float64: L = max(-log q, 0), and +inf (never reached) where q <= 0 or q is NaN.  Both backends compare
    against these very bits, so they cannot disagree on the entry a quantile falls in because of a logarithm."""
    q = quantiles.detach().to(torch.float64).reshape(num_rays, num_q)
    never = (q <= 0) | torch.isnan(q)
    level = (-torch.log(torch.where(never, torch.ones_like(q), q))).clamp_min(0.0)
    return torch.where(never, torch.full_like(q, float("inf")), level).contiguous()


def _ray_quantiles_torch(offsets, t_enter, t_exit, sigma, levels):
    """The definition: float64 throughout, one cumulative sum of x over the whole list, per quantile one
    ``searchsorted`` for the sum in front of the ray plus the level, gathers for t_enter[j], X_j and sigma[j].  Autograd
    differentiates it.  ``offsets`` and ``levels`` are on the device of ``sigma``."""
    dev, dtype = sigma.device, sigma.dtype
    total = sigma.size(0)
    if total == 0:
        return (torch.full(levels.shape, -1.0, dtype=dtype, device=dev),
                torch.full(levels.shape, -1, dtype=torch.int64, device=dev))
    t_enter = t_enter.to(dev).to(torch.float64).reshape(-1)
    t_exit = t_exit.to(dev).to(torch.float64).reshape(-1)
    dt = torch.where(torch.isinf(t_exit), torch.zeros_like(t_exit), (t_exit - t_enter).clamp_min(0.0))
    density = sigma.to(torch.float64)
    x = density * dt
    run0 = torch.cat([x.new_zeros(1), torch.cumsum(x, 0)])         # run0[e] = sum of the entries before e
    first = run0[offsets[:-1]].unsqueeze(-1)                       # [R, 1]: the sum in front of each ray's first entry
    # the first entry whose inclusive sum exceeds first + L: at or behind the ray's first entry, as L >= 0
    j = torch.searchsorted(run0.detach()[1:].contiguous(), (first.detach() + levels).contiguous(), right=True)
    valid = j < offsets[1:].unsqueeze(-1)
    at = torch.where(valid, j, torch.zeros_like(j))
    # selected before the division: a pair without a crossing divides 0 by 1, and no 0 * inf reaches a gradient
    remaining = torch.where(valid, levels - (run0[at] - first), torch.zeros_like(levels))
    density_at = torch.where(valid, density[at], torch.ones_like(levels))
    depth = torch.where(valid, t_enter[at] + remaining / density_at, torch.full_like(levels, -1.0))
    return depth.to(dtype), torch.where(valid, j, torch.full_like(j, -1))


class _RayQuantiles(torch.autograd.Function):
    """``ray_quantiles`` through the kernels of rf_quantiles.hip: float32 CUDA tensors, each gradient only where its
    input needs one.  The inputs, the levels and the entries of the forward are kept for the backward, which sweeps the
    list once more."""

    @staticmethod
    def forward(ctx, sigma, t_enter, t_exit, levels, offsets):

        dev = sigma.device
        num_rays, total, num_q = offsets.numel() - 1, sigma.size(0), levels.size(1)
        if num_rays >= 2 ** 31:
            raise RuntimeError("too many rays for the kernel")
        offsets = offsets.to(dev).contiguous()
        sigma_c = sigma.detach().contiguous()
        t_enter_c, t_exit_c = _times_for_kernel(ctx, dev, t_enter, t_exit)
        if num_rays == 0 or total == 0:
            depth = torch.full((num_rays, num_q), -1.0, dtype=torch.float32, device=dev)
            entries = torch.full((num_rays, num_q), -1, dtype=torch.int64, device=dev)
        else:
            depth = torch.empty((num_rays, num_q), dtype=torch.float32, device=dev)      # every element is written
            entries = torch.empty((num_rays, num_q), dtype=torch.int64, device=dev)
            with torch.cuda.device(dev):
                rc = _lib.load().rf_ray_quantiles_forward(
                    num_rays, _ptr(offsets), total, _ptr(t_enter_c), _ptr(t_exit_c), _ptr(sigma_c), num_q,
                    _ptr(levels), _ptr(depth), _ptr(entries), _stream(dev))
            _lib.check(rc)
        ctx.save_for_backward(sigma_c, t_enter_c, t_exit_c, offsets, levels, entries)
        ctx.mark_non_differentiable(entries)
        return depth, entries

    @staticmethod
    def backward(ctx, grad_depth, _grad_entries):

        sigma, t_enter, t_exit, offsets, levels, entries = ctx.saved_tensors
        dev = sigma.device
        num_rays, total, num_q = offsets.numel() - 1, sigma.size(0), levels.size(1)
        want = ctx.needs_input_grad[:3]
        # entries outside offsets[0] .. offsets[R] are not written by the kernel: there are none in a sound list
        grads = [torch.empty_like(sigma) if w else None for w in want]
        if num_rays > 0 and total > 0 and any(want):
            grad_depth = grad_depth.to(torch.float32).contiguous()
            with torch.cuda.device(dev):
                rc = _lib.load().rf_ray_quantiles_backward(
                    num_rays, _ptr(offsets), total, _ptr(t_enter), _ptr(t_exit), _ptr(sigma), num_q, _ptr(levels),
                    _ptr(entries), _ptr(grad_depth), _ptr(grads[0]), _ptr(grads[1]), _ptr(grads[2]), _stream(dev))
            _lib.check(rc)
        return (grads[0], *_times_grads(ctx, grads[1], grads[2]), None, None)


def ray_quantiles(seg, sigma: torch.Tensor, quantiles: torch.Tensor, backend=None):
    """(depth [R, Q], entries [R, Q] int64): where along each ray of ``seg`` (the dict ``Pipeline.trace_segments`` or
    ``trace_differentiable_segments`` returns; ``offsets`` int64 [R+1] and ``t_enter`` / ``t_exit`` [S] are read,
    ``cells`` is not) the transmittance of a density ``sigma`` [S] PER ENTRY, float32 or float64, falls through the
    levels ``quantiles`` [R, Q] (any shape with R Q elements whose last dimension is Q; dtype and device of ``sigma``):
    the ``depth`` output of ``trace_forward(depth_quantiles=...)`` for a density of one's own.  q = 0.5 is the median
    depth; ``|depth[:, 0] - depth[:, 1]|`` on two random quantiles is the reference's regulariser
    (examples/quantile_regulariser.py); ``seg["cells"][entries]`` are the reference's ``quantile_point_indices``.  Per
    ray, over its entries in order, in double:

        dt = 0 where t_exit is infinite, else max(t_exit - t_enter, 0),      x = sigma dt
        X_i = sum of x over the ray's earlier entries,      I_i = X_i + x_i
        L = max(-log(quantile), 0);  +inf (never reached) where the quantile is <= 0 or NaN
        j = the first entry of the ray with I_j > L
        depth = t_enter[j] + (L - X_j) / sigma[j],      entries = j, an index into the list

    and depth = -1, entries = -1 where the ray has no such entry: the quantile lies below the ray's final
    transmittance, or the ray has no entries.  Every quantile is found on its own; for a row sorted in descending order
    this is what the reference's sequential loop gives.  A quantile >= 1 behaves as 1: its depth is ``t_enter`` of the
    first entry with x > 0.  ``sigma >= 0`` is a precondition (negative densities give unspecified values).  The result
    has the dtype of ``sigma``.

    Differentiable in ``sigma``, ``seg["t_enter"]`` and ``seg["t_exit"]`` (which carry the gradient on to the points and
    the rays when they come from ``trace_differentiable_segments``), not in ``quantiles``; ``entries`` is marked
    non-differentiable.  The entry a quantile falls in is held fixed.  The times' gradient follows torch's
    ``clamp_min``: an entry with t_exit >= t_enter, both finite, passes it on; an entry with an infinite t_exit gets
    exact zeros in every gradient; ``t_exit`` of the crossing entry gets nothing.

    ``backend``: None, "hip" or "torch", as in ``composite_entries``.  None is "hip" for float32 CUDA ``sigma`` with at
    most ``rf_quantiles_max()`` (8) quantiles per ray and "torch" for everything else; "hip" with more quantiles raises.
    "hip" runs the kernels of rf_quantiles.hip (one wave owns a run of consecutive rays, a segmented scan in double, one
    rounding to float32, no atomics: the same bits from call to call, gradients included; the times are read as
    float32).  "torch" restates the definition in float64 with one list-wide cumulative sum and a ``searchsorted`` per
    quantile, differentiated by autograd, on any device; no Python loop over rays.  The levels L are formed here, in
    float64, for both backends.  ``offsets[-1] == S`` is checked on the torch path only, and there only when
    ``seg["offsets"]`` lives on the CPU.  (The kernels clamp every offset to 0 .. S instead.)"""
    num_rays, total, num_q = _check_quantiles_inputs(seg, sigma, quantiles)
    chosen = _choose_backend(backend, sigma, "sigma")
    if chosen == "hip":
        most =int(_lib.load().rf_quantiles_max())
        if num_q > most and backend is None:
            chosen = "torch"
        elif num_q > most:
            raise RuntimeError(f"the kernel takes at most {most} quantiles per ray (backend='torch' takes any number)")
    levels = _quantile_levels(quantiles, num_rays, num_q)
    if chosen == "torch":
        if not seg["offsets"].is_cuda and int(seg["offsets"][-1]) != total:
            raise RuntimeError("seg['offsets'][-1] must be the number of entries")
        return _ray_quantiles_torch(seg["offsets"].to(sigma.device), seg["t_enter"], seg["t_exit"], sigma, levels)
    return _RayQuantiles.apply(sigma, seg["t_enter"], seg["t_exit"], levels, seg["offsets"])


def _check_weights_inputs(seg, sigma):
    if sigma.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("sigma must have float32 or float64 dtype")
    if sigma.dim() != 1:
        raise RuntimeError("expected sigma [S]")
    offsets = _check_offsets(seg["offsets"])
    total = sigma.size(0)
    if seg["t_enter"].numel() != total or seg["t_exit"].numel() != total:
        raise RuntimeError("sigma, seg['t_enter'] and seg['t_exit'] must have one element per entry")
    return offsets.numel() - 1, total


def _entry_weights_torch(offsets, t_enter, t_exit, sigma):
    """The definition with the operations of ``_composite_entries_torch``, stopping before its ``index_add``: float64
    throughout, the sum over a ray's earlier entries as a difference of one list-wide cumulative sum.  Autograd
    differentiates it.  ``offsets`` is on the device of ``sigma``.  Returns (weights, transmittance)."""
    dev, dtype = sigma.device, sigma.dtype
    t_enter = t_enter.to(dev).to(torch.float64).reshape(-1)
    t_exit = t_exit.to(dev).to(torch.float64).reshape(-1)
    dt = torch.where(torch.isinf(t_exit), torch.zeros_like(t_exit), (t_exit - t_enter).clamp_min(0.0))
    log_keep = -sigma.to(torch.float64) * dt                       # -x = log(1 - alpha) of every entry
    log_before = _sums_in_ray(log_keep, offsets, _entry_rays(offsets, sigma.size(0)))[0]
    transmittance = torch.exp(log_before)                          # exp(0) = 1 at every ray's first entry
    return (transmittance * -torch.expm1(log_keep)).to(dtype), transmittance.to(dtype)


class _EntryWeights(torch.autograd.Function):
    """``entry_weights`` through the kernels of rf_entry_weights.hip: float32 CUDA tensors, each gradient only where its
    input needs one, and an output nobody used costs neither a zero tensor nor a read.  Nothing but the inputs is kept
    for the backward, which sweeps the list twice."""

    @staticmethod
    def forward(ctx, sigma, t_enter, t_exit, offsets, with_transmittance):

        dev = sigma.device
        num_rays, total = offsets.numel() - 1, sigma.size(0)
        if num_rays >= 2 ** 31:
            raise RuntimeError("too many rays for the kernel")
        offsets = offsets.to(dev).contiguous()
        sigma_c = sigma.detach().contiguous()
        t_enter_c, t_exit_c = _times_for_kernel(ctx, dev, t_enter, t_exit)
        ctx.save_for_backward(sigma_c, t_enter_c, t_exit_c, offsets)
        ctx.set_materialize_grads(False)
        # entries outside offsets[0] .. offsets[R] are not written by the kernel: there are none in a sound list
        new = torch.empty_like if num_rays > 0 and total > 0 else torch.zeros_like
        weights = new(sigma_c)
        transmittance = new(sigma_c) if with_transmittance else None
        if num_rays > 0 and total > 0:
            with torch.cuda.device(dev):
                rc = _lib.load().rf_entry_weights_forward(
                    num_rays, _ptr(offsets), total, _ptr(t_enter_c), _ptr(t_exit_c), _ptr(sigma_c), _ptr(weights),
                    _ptr(transmittance), _stream(dev))
            _lib.check(rc)
        return (weights, transmittance) if with_transmittance else weights

    @staticmethod
    def backward(ctx, grad_weights, grad_transmittance=None):

        sigma, t_enter, t_exit, offsets = ctx.saved_tensors
        dev = sigma.device
        num_rays, total = offsets.numel() - 1, sigma.size(0)
        want = ctx.needs_input_grad[:3]
        runs = num_rays > 0 and total > 0 and any(want)
        new = torch.empty_like if runs else torch.zeros_like
        grads = [new(sigma) if w else None for w in want]
        if runs:
            g_w, g_t = (None if g is None else g.to(torch.float32).contiguous()
                        for g in (grad_weights, grad_transmittance))             # None: zeros, and not read
            with torch.cuda.device(dev):
                rc = _lib.load().rf_entry_weights_backward(
                    num_rays, _ptr(offsets), total, _ptr(t_enter), _ptr(t_exit), _ptr(sigma), _ptr(g_w), _ptr(g_t),
                    _ptr(grads[0]), _ptr(grads[1]), _ptr(grads[2]), _stream(dev))
            _lib.check(rc)
        return (grads[0], *_times_grads(ctx, grads[1], grads[2]), None, None)


def entry_weights(seg, sigma: torch.Tensor, return_transmittance=False, backend=None):
    """weights [S], or (weights [S], transmittance [S]) with ``return_transmittance``: the compositing weight of every
    entry of ``seg`` (the dict ``Pipeline.trace_segments`` or ``trace_differentiable_segments`` returns; ``offsets``
    int64 [R+1] and ``t_enter`` / ``t_exit`` [S] are read, ``cells`` is not) and the transmittance in front of it, for a
    density ``sigma`` [S] PER ENTRY, float32 or float64.  Per ray, over its entries in order (the
    definitions of ``composite_entries`` word for word):

        dt = 0 where t_exit is infinite, else max(t_exit - t_enter, 0),      x = sigma dt
        T = exp(-(sum of x over the ray's earlier entries))          transmittance
        w = T (1 - exp(-x))                                          weights

    ``composite_entries`` is the sum of ``w values`` per ray; this is for everything that is not linear in the weights:
    the ray entropy ``-sum w log w`` (examples/weight_entropy.py), a proposal loss between two densities on one walk, a
    per-entry visibility T, the largest weight a cell ever gets, weight times error per cell through
    ``reduce_entries``.  T is exactly 1 at every ray's first entry and w is exactly 0 behind an infinite ``t_exit``.
    The results have the dtype and device of ``sigma``.

    Differentiable in ``sigma``, ``seg["t_enter"]`` and ``seg["t_exit"]`` (which carry the gradient on to the points and
    the rays when they come from ``trace_differentiable_segments``).  The times' gradient follows torch's
    ``clamp_min``: an entry with t_exit >= t_enter, both finite, passes it on, t_exit < t_enter does not, and an entry
    with an infinite t_exit gets exact zeros in every gradient.

    ``backend``: None, "hip" or "torch", as in ``composite_entries``.  None is "hip" for float32 CUDA ``sigma`` and
    "torch" for everything else.  "hip" runs the kernels of rf_entry_weights.hip (one wave owns a run of consecutive
    rays, a segmented scan in double, one rounding to float32, no atomics: the same bits from call to call, gradients
    included; the times are read as float32; an output that the loss does not use is not read back in the backward).
    "torch" restates the definition in float64 with one list-wide cumulative sum, differentiated by autograd, on any
    device; no Python loop over rays.  ``offsets[-1] == S`` is checked on the torch path only, and there only when
    ``seg["offsets"]`` lives on the CPU.  (The kernels clamp every offset to 0 .. S instead.)"""
    _check_weights_inputs(seg, sigma)
    if _choose_backend(backend, sigma, "sigma") == "torch":
        if not seg["offsets"].is_cuda and int(seg["offsets"][-1]) != sigma.size(0):
            raise RuntimeError("seg['offsets'][-1] must be the number of entries")
        weights, transmittance = _entry_weights_torch(seg["offsets"].to(sigma.device), seg["t_enter"], seg["t_exit"],
                                                      sigma)
        return (weights, transmittance) if return_transmittance else weights
    return _EntryWeights.apply(sigma, seg["t_enter"], seg["t_exit"], seg["offsets"], bool(return_transmittance))


_NONE = 0xFFFFFFFF


def _check_segment_grad_inputs(seg, exit_cells, points, rays, grad_t_enter, grad_t_exit):
    if points.dim() != 2 or points.size(-1) != 3:
        raise RuntimeError("expected points [N, 3]")
    if points.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("points must have float32 or float64 dtype")
    offsets = _check_offsets(seg["offsets"])
    num_rays, total = offsets.numel() - 1, seg["cells"].numel()
    if seg["t_enter"].numel() != total or seg["t_exit"].numel() != total:
        raise RuntimeError("seg['cells'], seg['t_enter'] and seg['t_exit'] must have one element per entry")
    if grad_t_enter.numel() != total or grad_t_exit.numel() != total:
        raise RuntimeError("grad_t_enter and grad_t_exit must have one element per entry")
    if exit_cells.numel() != num_rays:
        raise RuntimeError("exit_cells must have one element per ray")
    if rays.size(-1) != 6 or rays.numel() != 6 * num_rays:
        raise RuntimeError("rays must have one row of 6 per ray")
    return num_rays, total


def _segment_face_totals(seg, exit_cells, dev, dtype, grad_t_enter, grad_t_exit, num_rays, total):
    """What both restatements share: per entry the ray index, the cell, the cell behind its face (0 where
    there is none), whether there is one, and the holder-aware total G, in ``dtype`` on ``dev``."""
    offsets = seg["offsets"].to(dev)
    cells = seg["cells"].to(dev).to(torch.int64)
    t_enter, t_exit = seg["t_enter"].to(dev), seg["t_exit"].to(dev)      # holders: from the stored floats
    g_enter, g_exit = grad_t_enter.to(dev).to(dtype).reshape(-1), grad_t_exit.to(dev).to(dtype).reshape(-1)
    exits = exit_cells.to(dev).to(torch.int64) & _NONE
    ray = _entry_rays(offsets, total)
    index = torch.arange(total, device=dev)

    # the cell behind face j: the next entry, or exit_cells behind a ray's last entry; none behind an infinite exit
    last = index == offsets[1:][ray] - 1
    after = torch.where(last, exits[ray], torch.cat([cells[1:], cells.new_zeros(1)]))
    has_next = torch.isfinite(t_exit) & (after != _NONE)

    # t_enter[m] is the t_exit of the last holder in front of m within the ray (0, a constant, when there is none)
    holder = t_exit > t_enter
    latest = torch.cummax(torch.where(holder, index, index.new_full((), -1)), 0).values
    held_by = torch.cat([latest.new_full((1,), -1), latest[:-1]])
    owned = held_by >= offsets[:-1][ray]
    total_grad = g_exit.index_add(0, held_by.clamp_min(0), torch.where(owned, g_enter, torch.zeros_like(g_enter)))
    return ray, cells, torch.where(has_next, after, torch.zeros_like(after)), has_next, total_grad


def _segment_points_grad_torch(seg, exit_cells, points, rays, grad_t_enter, grad_t_exit, num_rays, total):
    """DESIGN 4.9, restated with torch operations over all S entries at once, in the dtype of ``points``."""
    dev, dtype = points.device, points.dtype
    out = torch.zeros_like(points)
    if total == 0:
        return out
    ray, cells, after, has_next, total_grad = _segment_face_totals(
        seg, exit_cells, dev, dtype, grad_t_enter, grad_t_exit, num_rays, total)

    live = has_next & (total_grad != 0)                                   # G == 0 exactly adds nothing: no 0 * inf
    r = rays.to(dev).reshape(-1, 6).to(dtype)
    origin = r[:, :3][ray]
    direction = (r[:, 3:] / (r[:, 3:] * r[:, 3:]).sum(-1, keepdim=True).sqrt())[ray]
    pa = points.detach()[cells]
    pb = points.detach()[after]
    normal = pb - pa
    num = (((pa + pb) / 2 - origin) * normal).sum(-1, keepdim=True)
    dp = (normal * direction).sum(-1, keepdim=True)
    den = dp * dp
    weight = total_grad.unsqueeze(-1)
    zero = torch.zeros_like(pa)
    live = live.unsqueeze(-1)
    grad_a = torch.where(live, weight * ((num * direction + dp * (origin - pa)) / den), zero)
    grad_b = torch.where(live, weight * (-(num * direction + dp * (origin - pb)) / den), zero)
    out.index_add_(0, cells, grad_a)
    out.index_add_(0, after, grad_b)
    return out


def _segment_rays_grad_torch(seg, exit_cells, points, rays, grad_t_enter, grad_t_exit, num_rays, total):
    """DESIGN 4.10, restated with torch operations over all S entries at once, in the dtype of ``points``."""
    dev, dtype = points.device, points.dtype
    out = torch.zeros((num_rays, 6), dtype=dtype, device=dev)
    if total == 0:
        return out
    ray, cells, after, has_next, total_grad = _segment_face_totals(
        seg, exit_cells, dev, dtype, grad_t_enter, grad_t_exit, num_rays, total)

    live = (has_next & (total_grad != 0)).unsqueeze(-1)                   # G == 0 exactly adds nothing: no 0 * inf
    r = rays.detach().to(dev).reshape(-1, 6).to(dtype)
    length = (r[:, 3:] * r[:, 3:]).sum(-1, keepdim=True).sqrt()
    origin = r[:, :3][ray]
    direction = (r[:, 3:] / length)[ray]
    pa = points.detach()[cells]
    pb = points.detach()[after]
    normal = pb - pa
    num = (((pa + pb) / 2 - origin) * normal).sum(-1, keepdim=True)
    dp = (normal * direction).sum(-1, keepdim=True)
    weight = total_grad.unsqueeze(-1)
    to_origin = -(weight / dp) * normal
    to_direction = -(weight * num / (dp * dp * length[ray])) * (normal - dp * direction)
    both = torch.cat([to_origin, to_direction], dim=-1)
    out.index_add_(0, ray, torch.where(live, both, torch.zeros_like(both)))
    return out


def segment_points_grad(seg, exit_cells, points, rays, grad_t_enter, grad_t_exit, backend=None) -> torch.Tensor:
    """dL/dpoints [N, 3] from dL/dt_enter [S] and dL/dt_exit [S] of the walk ``seg`` (the dict
    ``Pipeline.trace_differentiable_segments`` returns; ``exit_cells`` uint32 [R] is its entry of that name: the cell
    behind every ray's last face, 0xFFFFFFFF for none).  DESIGN 4.9:

        face j lies between a = cells[j] and b = the next cell of the walk; none where t_exit[j] is infinite
        j holds the running maximum iff t_exit[j] > t_enter[j] (the stored floats decide)
        G_j = grad_t_exit[j] + [j holds] * sum of grad_t_enter over the ray's later entries up to the next holder, included
        points_grad[a] += G_j dt/dp_a,  points_grad[b] += G_j dt/dp_b         (nothing where G_j == 0 exactly)

    with t the crossing of the ray (origin, normalised direction) and the exact bisector of (p_a, p_b) -- the
    derivative ``trace_backward`` uses, not that of the fp16 face table the walk ran on.  The gradient of t_enter in
    front of a ray's first holder is dropped (t_enter is the constant 0 there).  The rays' gradient is
    ``segment_rays_grad``'s; a grazing face may give non-finite values, as in ``trace_backward``.

    CUDA tensors go through the HIP kernel (float32 points; one lane per entry, atomics into a zeroed [N, 3]).  CPU
    tensors, and CUDA tensors with ``backend="torch"``, go through a vectorised torch restatement in the dtype of
    ``points`` (float32 or float64): no Python loop over rays."""
    num_rays, total = _check_segment_grad_inputs(seg, exit_cells, points, rays, grad_t_enter, grad_t_exit)
    if _choose_backend(backend, points, "points", any_dtype=True) == "torch":
        return _segment_points_grad_torch(seg, exit_cells, points, rays, grad_t_enter, grad_t_exit, num_rays, total)
    out = torch.zeros((points.size(0), 3), dtype=torch.float32, device=points.device)
    return _segment_grad_hip("rf_segments_points_grad", out, seg, exit_cells, points, rays, grad_t_enter, grad_t_exit,
                             num_rays, total)


def _segment_grad_hip(symbol, out, seg, exit_cells, points, rays, grad_t_enter, grad_t_exit, num_rays, total):
    """The launch both gradient kernels share: ``symbol`` accumulates into the zeroed ``out``."""

    dev = points.device
    if total == 0 or points.size(0) == 0 or num_rays == 0:
        return out
    if num_rays >= 2 ** 31:
        raise RuntimeError("too many rays for an int32 ray index")

    def f32(t):
        return t.detach().to(dev).to(torch.float32).reshape(-1).contiguous()

    points_c = points.detach().contiguous()
    rays_c = rays.detach().to(dev).to(torch.float32).reshape(-1, 6).contiguous()
    offsets = seg["offsets"].to(dev).contiguous()
    cells = seg["cells"].to(dev).contiguous()
    exits = exit_cells.to(dev).contiguous()
    if cells.dtype != torch.uint32 or exits.dtype != torch.uint32:
        raise RuntimeError("seg['cells'] and exit_cells must have uint32 dtype")
    t_enter, t_exit = f32(seg["t_enter"]), f32(seg["t_exit"])
    g_enter, g_exit = f32(grad_t_enter), f32(grad_t_exit)
    entry_ray = _entry_rays(offsets, total, dtype=torch.int32)
    with torch.cuda.device(dev):
        rc = getattr(_lib.load(), symbol)(
            points_c.size(0), _ptr(points_c), num_rays, _ptr(rays_c), _ptr(offsets), total, _ptr(entry_ray),
            _ptr(cells), _ptr(t_enter), _ptr(t_exit), _ptr(exits), _ptr(g_enter), _ptr(g_exit), _ptr(out),
            _stream(dev))
    _lib.check(rc)
    return out


def segment_rays_grad(seg, exit_cells, points, rays, grad_t_enter, grad_t_exit, backend=None) -> torch.Tensor:
    """dL/drays [R, 6] from dL/dt_enter [S] and dL/dt_exit [S] of the walk ``seg``: the other half of what the stored
    times depend on (arguments of ``segment_points_grad``).  DESIGN 4.10, in the terms of 4.9 (a = cells[j], b = the
    next cell, G_j the holder-aware total) and with n = p_b - p_a, m = (p_a + p_b) / 2, O the origin, D the stored
    direction, d = D / |D|, num = (m - O) . n, dp = n . d:

        ray_grad[r, 0:3] = sum over the ray's entries of G_j * (-n / dp)
        ray_grad[r, 3:6] = sum over the ray's entries of G_j * (-num / (dp^2 |D|)) * (n - dp d)

    the derivative of the crossing t = num / dp of the exact fp32 bisector with the cell sequence and the start cell
    held fixed.  The second line has no component along D (scaling D changes nothing).  Faces with G_j == 0 exactly, or
    without a next cell, add nothing; there is no guard beyond that: dp = 0 gives non-finite values in that ray's row.

    CUDA tensors go through the HIP kernel (float32 points; one lane per entry, a segmented reduction in double within
    the wave, one atomic update of a ray's row per wave the ray reaches into).  CPU tensors, and CUDA tensors with
    ``backend="torch"``, go through a vectorised torch restatement in the dtype of ``points`` (float32 or float64): no
    Python loop over rays."""
    num_rays, total = _check_segment_grad_inputs(seg, exit_cells, points, rays, grad_t_enter, grad_t_exit)
    if _choose_backend(backend, points, "points", any_dtype=True) == "torch":
        return _segment_rays_grad_torch(seg, exit_cells, points, rays, grad_t_enter, grad_t_exit, num_rays, total)
    out = torch.zeros((num_rays, 6), dtype=torch.float32, device=points.device)
    return _segment_grad_hip("rf_segments_rays_grad", out, seg, exit_cells, points, rays, grad_t_enter, grad_t_exit,
                             num_rays, total)


class _SegmentTimes(torch.autograd.Function):
    """t_enter / t_exit of a walk as functions of the points and the rays: the forward hands back the stored tensors,
    the backward is ``segment_points_grad`` and ``segment_rays_grad``, each only where its input needs a gradient."""

    @staticmethod
    def forward(ctx, points, rays, offsets, cells, exit_cells, t_enter, t_exit):
        ctx.save_for_backward(points, rays, offsets, cells, exit_cells, t_enter, t_exit)
        return t_enter, t_exit

    @staticmethod
    def backward(ctx, grad_t_enter, grad_t_exit):
        points, rays, offsets, cells, exit_cells, t_enter, t_exit = ctx.saved_tensors
        seg = {"offsets": offsets, "cells": cells, "t_enter": t_enter, "t_exit": t_exit}
        grad_t_enter = torch.zeros_like(t_enter) if grad_t_enter is None else grad_t_enter
        grad_t_exit = torch.zeros_like(t_exit) if grad_t_exit is None else grad_t_exit
        grad_points = grad_rays = None
        if ctx.needs_input_grad[0]:
            grad_points = segment_points_grad(seg, exit_cells, points, rays, grad_t_enter, grad_t_exit).to(points.dtype)
        if ctx.needs_input_grad[1]:
            grad_rays = segment_rays_grad(seg, exit_cells, points, rays, grad_t_enter, grad_t_exit)
            grad_rays = grad_rays.to(rays.dtype).reshape(rays.shape)
        return grad_points, grad_rays, None, None, None, None, None
