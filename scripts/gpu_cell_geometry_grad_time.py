"""Time of radfoam.cell_geometry_grad (the kernels of rf_cell_geometry_grad.hip) next to radfoam.cell_geometry on the
cloud of DESIGN 4.7: 2 M points uniform in [-1,1]^3 (seed 0) triangulated on the GPU.  HIP events around the whole Python
call (kernels, bbox, status read-back), 3 warm-up calls, median (min, max) of 5.  The upstreams are random on the
bounded cells; ``backward`` is forward plus backward through differentiable_cell_geometry.

    python scripts/gpu_cell_geometry_grad_time.py [--points 2000000]      # prints one JSON line
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import radfoam
from radfoam_amd.triangulation import Triangulation

N = int(sys.argv[sys.argv.index("--points") + 1]) if "--points" in sys.argv else 2000000
dev = "cuda:0"
gen = torch.Generator(device="cpu").manual_seed(0)
pts = (torch.rand((N, 3), generator=gen) * 2.0 - 1.0).to(dev)
tri = Triangulation(pts)
p = pts[tri.permutation().to(torch.int64)].contiguous()
adj, off = tri.point_adjacency(), tri.point_adjacency_offsets()
rows = (off[1:].to(torch.int64) - off[:-1].to(torch.int64))
print("triangulated", N, int(adj.numel()), int(rows.max()), flush=True)


def timed(fn, reps=5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return [float(np.median(out)), float(min(out)), float(max(out))]


geo = radfoam.cell_geometry(p, adj, off)
g = torch.Generator(device=dev).manual_seed(1)
gv = torch.rand(N, dtype=torch.float64, device=dev, generator=g) * 2 - 1
gc = torch.rand((N, 3), dtype=torch.float64, device=dev, generator=g) * 2 - 1
grad = radfoam.cell_geometry_grad(p, adj, off, geo, gv, gc)
assert bool(torch.isfinite(grad).all())


def forward_backward():
    q = p.clone().requires_grad_(True)
    out = radfoam.differentiable_cell_geometry(q, adj, off)
    b = out.bounded
    (out.volume[b].sum() + out.centroid[b].sum()).backward()


res = {"points": N, "edges": int(adj.numel()), "longest_row": int(rows.max()), "bounded": int(geo.bounded.sum()),
       "cell_geometry_ms": timed(lambda: radfoam.cell_geometry(p, adj, off)),
       "cell_geometry_grad_ms": timed(lambda: radfoam.cell_geometry_grad(p, adj, off, geo, gv, gc)),
       "cell_geometry_grad_volume_only_ms": timed(lambda: radfoam.cell_geometry_grad(p, adj, off, geo, gv, None)),
       "differentiable_forward_backward_ms": timed(forward_backward)}
print(json.dumps(res))
