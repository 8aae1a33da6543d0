"""Time of Pipeline.trace_segments against trace_forward on the same rays: HIP events around the Python calls, 3 warm-up
calls, median (min, max) of 10.  trace_segments includes its prefix sum, its host synchronisation and the allocation of
the ragged outputs.

    python scripts/gpu_segments_time.py          # prints one JSON line
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
start = torch.full(rays.shape[:-1], foam.nearest_point(fm["points"], cam["position"]), dtype=torch.int64, device=dev).to(torch.uint32)
pipe = radfoam.create_pipeline(D)
pipe.record_trail = False

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

fwd = timed(lambda: pipe.trace_forward(p, a, adj, off, rays, start))
pipe.forward_mode = 3
fwd_strict = timed(lambda: pipe.trace_forward(p, a, adj, off, rays, start))
pipe.forward_mode = 0
seg = timed(lambda: pipe.trace_segments(p, a, adj, off, rays, start))
s = pipe.trace_segments(p, a, adj, off, rays, start)
res = {"points": N, "rays": W * H, "sh_degree": D, "entries": int(s["cells"].numel()),
       "trace_forward_ms": fwd, "trace_forward_strict_scan_ms": fwd_strict, "trace_segments_ms": seg}
print(json.dumps(res))
