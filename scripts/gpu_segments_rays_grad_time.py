"""Time of the rays gradient through an exported walk on the frame of scripts/gpu_segments_time.py: the
kernel behind radfoam.segment_rays_grad, its torch restatement (backend="torch") on the same device tensors, and
segment_points_grad (the kernel of DESIGN 4.9) for scale.  HIP events around the Python calls, 3 warm-up calls, median
(min, max) of 10.  The kernels' times include forming entry_ray (repeat_interleave) and zeroing the result.

    python scripts/gpu_segments_rays_grad_time.py          # prints one JSON line
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import radfoam
from radfoam_amd import foam

N, W, H, D = 100000, 960, 540, 2
t = time.time()
fm = foam.make_synthetic_foam(N, D, 1)
print("foam", time.time() - t, flush=True)
dev = "cuda:0"
p, a = torch.from_numpy(fm["points"]).to(dev), torch.from_numpy(fm["attributes"]).to(dev)
adj, off = torch.from_numpy(fm["point_adjacency"]).to(dev), torch.from_numpy(fm["point_adjacency_offsets"]).to(dev)
cam = foam.default_camera(W, H)
rays = torch.from_numpy(foam.camera_rays(cam)).to(dev)
nearest = foam.nearest_point(fm["points"], cam["position"])
start = torch.full(rays.shape[:-1], nearest, dtype=torch.int64, device=dev).to(torch.uint32)
pipe = radfoam.create_pipeline(D)

def timed(fn, reps=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), float(min(out)), float(max(out))

seg = pipe.trace_differentiable_segments(p, a, adj, off, rays, start)
total = seg["cells"].numel()
gen = torch.Generator(device=dev).manual_seed(0)
g_enter = torch.randn(total, device=dev, generator=gen)
g_exit = torch.randn(total, device=dev, generator=gen)
flat = rays.reshape(-1, 6)
kernel = timed(lambda: radfoam.segment_rays_grad(seg, seg["exit_cells"], p, flat, g_enter, g_exit))
print("kernel", kernel, flush=True)
restated = timed(lambda: radfoam.segment_rays_grad(seg, seg["exit_cells"], p, flat, g_enter, g_exit, backend="torch"))
print("restated", restated, flush=True)
points_kernel = timed(lambda: radfoam.segment_points_grad(seg, seg["exit_cells"], p, flat, g_enter, g_exit))
got = radfoam.segment_rays_grad(seg, seg["exit_cells"], p, flat, g_enter, g_exit).double()
ref = radfoam.segment_rays_grad(seg, seg["exit_cells"], p.double(), flat, g_enter, g_exit, backend="torch")
finite = torch.isfinite(ref).all(dim=1) & torch.isfinite(got).all(dim=1)
rel = float((got[finite] - ref[finite]).norm() / ref[finite].norm())
res = {"points": N, "rays": W * H, "sh_degree": D, "entries": total,
       "segment_rays_grad_kernel_ms": kernel, "segment_rays_grad_torch_ms": restated,
       "segment_points_grad_kernel_ms": points_kernel,
       "kernel_vs_float64_rel_l2": rel, "rows_not_finite": int((~finite).sum())}
print(json.dumps(res))
