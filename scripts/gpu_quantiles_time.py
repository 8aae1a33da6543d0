"""Time and peak memory of radfoam.ray_quantiles (the kernels of rf_quantiles.hip) against its torch backend on the same
device tensors, on the frame of scripts/gpu_distortion_time.py (100,000 points, 960x540) with Q = 2 sorted random
quantiles per ray: HIP events around the Python calls, 3 warm-up calls, median (min, max) of 10.  Forward alone, then
forward plus backward of the quantile-gap loss into sigma, t_enter and t_exit.  Peak memory is
torch.cuda.max_memory_allocated over one call, above what the inputs hold; the gradients a backward returns are part of
it.  The GB/s figures divide the bytes the kernels must move (each input read once, each output written once) by the time
of the whole Python call, which includes forming the levels.

    python scripts/gpu_quantiles_time.py              # prints one JSON line
    python scripts/gpu_quantiles_time.py --hip-only   # the kernels alone (comparing builds of the library)
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import radfoam
from radfoam_amd import _lib, foam

N, W, H, D, Q = 100000, 960, 540, 2, 2
HIP_ONLY = "--hip-only" in sys.argv
t = time.time()
fm = foam.make_synthetic_foam(N, D, 1)
print("foam", time.time() - t, flush=True)
dev = "cuda:0"
p, a = torch.from_numpy(fm["points"]).to(dev), torch.from_numpy(fm["attributes"]).to(dev)
adj, off = torch.from_numpy(fm["point_adjacency"]).to(dev), torch.from_numpy(fm["point_adjacency_offsets"]).to(dev)
cam = foam.default_camera(W, H)
rays = torch.from_numpy(foam.camera_rays(cam)).to(dev)
start = torch.full(rays.shape[:-1], foam.nearest_point(fm["points"], cam["position"]), dtype=torch.int64, device=dev).to(torch.uint32)
pipe = radfoam.create_pipeline(D)
pipe.record_trail = False
seg = pipe.trace_segments(p, a, adj, off, rays, start)
R, S = W * H, int(seg["cells"].numel())
counts = seg["offsets"][1:] - seg["offsets"][:-1]
sigma = a[:, -1].float()[seg["cells"].to(torch.int64)].contiguous()
quantiles = torch.rand((R, Q), generator=torch.Generator().manual_seed(1)).sort(dim=-1, descending=True).values.to(dev)


def timed(fn, reps=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    torch.cuda.synchronize()
    getattr(fn, "reset", lambda: None)()          # the gradients of the call before count as the call's, not as inputs
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    return {"ms": [float(np.median(out)), float(min(out)), float(max(out))], "peak_mb": peak / 2 ** 20}


def gap(depth, entries):
    both = (entries >= 0).all(dim=-1)
    return torch.where(both, (depth[:, 0] - depth[:, 1]).abs(), torch.zeros_like(depth[:, 0])).sum()


def forward(**kw):
    return lambda: radfoam.ray_quantiles(seg, sigma, quantiles, **kw)


def forward_backward(**kw):
    leaf = lambda x: x.clone().requires_grad_(True)
    leaves = [leaf(sigma), leaf(seg["t_enter"]), leaf(seg["t_exit"])]

    def reset():
        for x in leaves:
            x.grad = None

    def fn():
        reset()
        gap(*radfoam.ray_quantiles({**seg, "t_enter": leaves[1], "t_exit": leaves[2]}, leaves[0], quantiles, **kw)).backward()
    fn.reset = reset
    return fn


res = {"points": N, "rays": R, "entries": S, "longest_ray": int(counts.max()), "quantiles": Q,
       "rays_per_wave": int(_lib.load().rf_quantiles_rays_per_wave())}
forward_bytes = 4 * 3 * S + 8 * (R + 1) + (8 + 4 + 8) * R * Q                   # levels in, depth and entries out
backward_bytes = 4 * 3 * S + 8 * (R + 1) + (8 + 8 + 4) * R * Q + 4 * 3 * S      # levels, entries, grad_depth in
with torch.no_grad():
    if not HIP_ONLY:
        res["forward_torch"] = timed(forward(backend="torch"))
    res["forward_hip"] = timed(forward())
if not HIP_ONLY:
    res["forward_backward_torch"] = timed(forward_backward(backend="torch"))
res["forward_backward_hip"] = timed(forward_backward())
res["forward_hip"]["gb_per_s"] = forward_bytes / res["forward_hip"]["ms"][0] / 1e6
res["forward_backward_hip"]["gb_per_s"] = (forward_bytes + backward_bytes) / res["forward_backward_hip"]["ms"][0] / 1e6
if not HIP_ONLY:                                  # how far the two backends are apart on this frame
    with torch.no_grad():
        (got, got_at), (want, want_at) = forward()(), forward(backend="torch")()
    same = got_at == want_at
    res["pairs_reached"] = int((want_at >= 0).sum())
    res["pairs_with_another_entry"] = int((~same).sum())
    diff = (got.double() - want.double()).abs()[same]
    res["largest_difference"] = float(diff.max())
    res["largest_difference_over_test_bound"] = float((diff / (1e-7 + 2e-7 * want.double().abs()[same])).max())
    res["largest_value"] = float(want.abs().max())
print(json.dumps(res))
