"""Time and peak memory of radfoam.ray_distortion (the kernels of rf_distortion.hip) against its torch backend on the
same device tensors, on the frame of scripts/gpu_composite_time.py (100,000 points, 960x540): HIP events around the
Python calls, 3 warm-up calls, median (min, max) of 10.  Forward alone, then forward plus backward through
.sum().backward() into sigma, t_enter and t_exit; both measured in t and in s = t / (1 + t) (then into s_enter and
s_exit as well).  Peak memory is torch.cuda.max_memory_allocated over one call, above what the inputs hold; the
gradients a backward returns are part of it.  The GB/s figures divide the bytes the kernels must move (each input read
once, each output written once) by the time of the whole Python call.

    python scripts/gpu_distortion_time.py              # prints one JSON line
    python scripts/gpu_distortion_time.py --hip-only   # the kernels alone (comparing builds of the library)
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

N, W, H, D = 100000, 960, 540, 2
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
finite = torch.isfinite(seg["t_exit"])
measure = (seg["t_enter"] / (1 + seg["t_enter"]),
           torch.where(finite, seg["t_exit"] / (1 + seg["t_exit"]), torch.ones_like(seg["t_exit"])))


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


def forward(own, **kw):
    s = measure if own else (None, None)
    return lambda: radfoam.ray_distortion(seg, sigma, s[0], s[1], **kw)


def forward_backward(own, **kw):
    leaf = lambda x: x.clone().requires_grad_(True)
    sig, t0, t1 = leaf(sigma), leaf(seg["t_enter"]), leaf(seg["t_exit"])
    s = (leaf(measure[0]), leaf(measure[1])) if own else (None, None)
    leaves = [sig, t0, t1] + ([s[0], s[1]] if own else [])

    def reset():
        for x in leaves:
            x.grad = None

    def fn():
        reset()
        radfoam.ray_distortion({**seg, "t_enter": t0, "t_exit": t1}, sig, s[0], s[1], **kw).sum().backward()
    fn.reset = reset
    return fn


res = {"points": N, "rays": R, "entries": S, "longest_ray": int(counts.max()),
       "rays_per_wave": int(_lib.load().rf_distortion_rays_per_wave())}
for own in (False, True):
    tag = "_s" if own else "_t"
    arrays = 5 if own else 3                      # [S] inputs; the backward writes as many [S] gradients
    forward_bytes = 4 * (arrays * S + R) + 8 * (R + 1)
    backward_bytes = 4 * (arrays * S + R + arrays * S) + 8 * (R + 1)       # the second sweep's reads: cache hits
    with torch.no_grad():
        if not HIP_ONLY:
            res["forward_torch" + tag] = timed(forward(own, backend="torch"))
        res["forward_hip" + tag] = timed(forward(own))
    if not HIP_ONLY:
        res["forward_backward_torch" + tag] = timed(forward_backward(own, backend="torch"))
    res["forward_backward_hip" + tag] = timed(forward_backward(own))
    res["forward_hip" + tag]["gb_per_s"] = forward_bytes / res["forward_hip" + tag]["ms"][0] / 1e6
    res["forward_backward_hip" + tag]["gb_per_s"] = (forward_bytes + backward_bytes) / res["forward_backward_hip" + tag]["ms"][0] / 1e6
if not HIP_ONLY:                                  # how far the two backends are apart on this frame, and the scale of the result
    with torch.no_grad():
        got, want = forward(False)().double(), forward(False, backend="torch")().double()
    res["largest_difference"] = float((got - want).abs().max())
    # the GPU tests' bar, 1e-7 + 2e-7 |reference|; at this size the float64 backend's list-wide sums are the coarser side
    res["largest_difference_over_test_bound"] = float(((got - want).abs() / (1e-7 + 2e-7 * want.abs())).max())
    res["largest_value"] = float(want.abs().max())
print(json.dumps(res))
