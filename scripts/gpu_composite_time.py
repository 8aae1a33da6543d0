"""Time and peak memory of radfoam.composite_entries (the kernels of rf_composite.hip) against its torch backend and
against composite_segments on the same device tensors, on the frame of scripts/gpu_segments_time.py (100,000 points,
960x540): HIP events around the Python calls, 3 warm-up calls, median (min, max) of 10.  Forward alone at C = 3, then
forward plus backward through .sum().backward() into sigma and values at C = 3 and C = 16.  Peak memory is
torch.cuda.max_memory_allocated over one call, above what the inputs hold.  The GB/s figures divide the bytes the
kernels must move (each input read once, each output written once) by the time of the whole Python call.

    python scripts/gpu_composite_time.py              # prints one JSON line
    python scripts/gpu_composite_time.py --hip-only   # the kernels alone (comparing builds of the library)
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
cells = seg["cells"].to(torch.int64)
gen = torch.Generator(device=dev).manual_seed(0)
density = a[:, -1].float().contiguous()
rgb = torch.rand((N, 3), device=dev, generator=gen)
sigma = density[cells].contiguous()


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


def forward_backward(values, **kw):
    s, v = sigma.clone().requires_grad_(True), values.clone().requires_grad_(True)

    def fn():
        s.grad = v.grad = None
        radfoam.composite_entries(seg, s, v, **kw).sum().backward()
    return fn


def segments_forward_backward():
    d, c = density.clone().requires_grad_(True), rgb.clone().requires_grad_(True)

    def fn():
        d.grad = c.grad = None
        radfoam.composite_segments(seg, d, c).sum().backward()
    return fn


res = {"points": N, "rays": R, "entries": S, "longest_ray": int(counts.max()),
       "rays_per_wave": int(_lib.load().rf_composite_rays_per_wave())}
with torch.no_grad():
    values3 = rgb[cells].contiguous()
    if not HIP_ONLY:
        res["forward_composite_segments"] = timed(lambda: radfoam.composite_segments(seg, density, rgb))
        res["forward_torch_c3"] = timed(lambda: radfoam.composite_entries(seg, sigma, values3, backend="torch"))
    res["forward_hip_c3"] = timed(lambda: radfoam.composite_entries(seg, sigma, values3))
if not HIP_ONLY:
    res["forward_backward_composite_segments"] = timed(segments_forward_backward())
for C in (3, 16):
    values = values3 if C == 3 else torch.rand((S, C), device=dev, generator=gen) * 2 - 1
    if not HIP_ONLY:
        res["forward_backward_torch_c%d" % C] = timed(forward_backward(values, backend="torch"))
    res["forward_backward_hip_c%d" % C] = timed(forward_backward(values))
    # forward: 3 [S] arrays per sweep of up to 4 channels, values once, out once; backward: 3 [S] arrays and values
    # (the second sweep's reads are counted as cache hits), G, and grad_sigma + grad_values written
    sweeps = (C + 3) // 4
    forward_bytes = 4 * (3 * S * sweeps + S * C + R * (C + 1)) + 8 * (R + 1) * sweeps
    backward_bytes = 4 * (3 * S + S * C + R * (C + 1) + S + S * C) + 8 * (R + 1)
    if C == 3:
        res["forward_hip_c3"]["gb_per_s"] = forward_bytes / res["forward_hip_c3"]["ms"][0] / 1e6
    res["forward_backward_hip_c%d" % C]["gb_per_s"] = (forward_bytes + backward_bytes) / res["forward_backward_hip_c%d" % C]["ms"][0] / 1e6
print(json.dumps(res))
