"""Time and peak memory of radfoam.entry_weights (the kernels of rf_entry_weights.hip) against the torch spelling it
replaces (its float64 torch backend, which is what examples/cell_statistics.py writes by hand, under autograd for the
backward) and against composite_entries at C = 1 (the sibling that does strictly more arithmetic) on the same device
tensors, on the frame of scripts/gpu_segments_time.py (100,000 points, 960x540): HIP events around the Python calls,
3 warm-up calls, median (min, max) of 10.  Forward alone (weights only, and both outputs), then forward plus backward
with both outputs used, through (w * a + T * b).sum().backward() into sigma.  Peak memory is
torch.cuda.max_memory_allocated over one call, above what the inputs hold.  The GB/s figures divide the bytes the
kernels must move (each input read once, each output written once) by the time of the whole Python call.

    python scripts/gpu_entry_weights_time.py              # prints one JSON line
    python scripts/gpu_entry_weights_time.py --hip-only   # the kernels alone (comparing builds of the library)
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
gen = torch.Generator(device=dev).manual_seed(0)
sigma = a[:, -1].float()[seg["cells"].to(torch.int64)].contiguous()
sigma64 = sigma.double()
ones = torch.rand((S, 1), device=dev, generator=gen)
g_w, g_t = torch.randn(S, device=dev, generator=gen), torch.randn(S, device=dev, generator=gen)


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
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    return {"ms": [float(np.median(out)), float(min(out)), float(max(out))], "peak_mb": peak / 2 ** 20}


def forward_backward(sig, **kw):
    s = sig.clone().requires_grad_(True)
    gw, gt = g_w.to(sig.dtype), g_t.to(sig.dtype)

    def fn():
        s.grad = None
        weights, through = radfoam.entry_weights(seg, s, return_transmittance=True, **kw)
        (weights * gw + through * gt).sum().backward()
    return fn


def composite_forward_backward():
    s = sigma.clone().requires_grad_(True)

    def fn():
        s.grad = None
        radfoam.composite_entries(seg, s, ones).sum().backward()
    return fn


res = {"points": N, "rays": R, "entries": S, "longest_ray": int(counts.max()),
       "rays_per_wave": int(_lib.load().rf_entry_weights_rays_per_wave())}
with torch.no_grad():
    if not HIP_ONLY:
        res["forward_torch_float64"] = timed(
            lambda: radfoam.entry_weights(seg, sigma64, return_transmittance=True, backend="torch"))
        res["forward_composite_c1"] = timed(lambda: radfoam.composite_entries(seg, sigma, ones))
    res["forward_hip_weights"] = timed(lambda: radfoam.entry_weights(seg, sigma))
    res["forward_hip_both"] = timed(lambda: radfoam.entry_weights(seg, sigma, return_transmittance=True))
if not HIP_ONLY:
    res["forward_backward_torch_float64"] = timed(forward_backward(sigma64, backend="torch"))
    res["forward_backward_composite_c1"] = timed(composite_forward_backward())
res["forward_backward_hip"] = timed(forward_backward(sigma))
# forward: 3 [S] arrays read, 1 or 2 written; backward: 3 [S] arrays and the 2 incoming gradients read (the second
# sweep's reads are counted as cache hits), grad_sigma written; the offsets once per launch
res["forward_hip_weights"]["gb_per_s"] = (4 * 4 * S + 8 * (R + 1)) / res["forward_hip_weights"]["ms"][0] / 1e6
res["forward_hip_both"]["gb_per_s"] = (4 * 5 * S + 8 * (R + 1)) / res["forward_hip_both"]["ms"][0] / 1e6
res["forward_backward_hip"]["gb_per_s"] = (4 * 11 * S + 16 * (R + 1)) / res["forward_backward_hip"]["ms"][0] / 1e6
print(json.dumps(res))
