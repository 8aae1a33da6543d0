"""Time of radfoam.cell_moments_grad (the kernels of rf_cell_moments_grad.hip) next to radfoam.cell_geometry_grad and
radfoam.cell_moments in the same run, on the cloud of DESIGN 4.7: 2 M points uniform in [-1,1]^3 (seed 0) triangulated on
the GPU.  HIP events around the whole Python call (kernels, bbox, status read-back), 3 warm-up calls, median (min, max)
of 5.  ``cell_moments_grad_ms`` is the operator alone with both upstreams, given the geometry; ``backward_ms`` is forward
plus backward of sum tr(site_moment) through differentiable_cell_moments.  There is no earlier implementation to compare
with: the figure to read is the ratio to cell_geometry_grad, which clips the same faces.

    python scripts/gpu_cell_moments_grad_time.py [--points 2000000]      # prints one JSON line
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
E = int(adj.numel())
print("triangulated", N, E, int(rows.max()), flush=True)


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
b = geo.bounded
gen = torch.Generator(device="cpu").manual_seed(1)
size = torch.where(b, geo.volume, torch.ones_like(geo.volume)) ** (4.0 / 3.0)
gq = ((torch.rand((N, 6), generator=gen, dtype=torch.float64) * 2.0 - 1.0).to(dev) / size[:, None]).contiguous()
gc = ((torch.rand((N, 6), generator=gen, dtype=torch.float64) * 2.0 - 1.0).to(dev) / size[:, None]).contiguous()
gv, gcen = torch.ones_like(geo.volume), torch.ones_like(geo.centroid)
grad = radfoam.cell_moments_grad(p, adj, off, geo, gq, gc)
assert bool(torch.isfinite(grad).all())


def backward():
    q = p.clone().requires_grad_(True)
    mo = radfoam.differentiable_cell_moments(q, adj, off)
    mo.site_moment[b][:, :3].sum().backward()
    return q.grad


res = {"points": N, "edges": E, "longest_row": int(rows.max()), "bounded_cells": int(b.sum()),
       "max_abs_grad": float(grad.abs().max()),
       "cell_geometry_grad_ms": timed(lambda: radfoam.cell_geometry_grad(p, adj, off, geo, gv, gcen)),
       "cell_moments_ms": timed(lambda: radfoam.cell_moments(p, adj, off, geo)),
       "cell_moments_grad_ms": timed(lambda: radfoam.cell_moments_grad(p, adj, off, geo, gq, gc)),
       "cell_moments_grad_site_only_ms": timed(lambda: radfoam.cell_moments_grad(p, adj, off, geo, gq)),
       "backward_ms": timed(backward)}
res["ratio_to_cell_geometry_grad"] = res["cell_moments_grad_ms"][0] / res["cell_geometry_grad_ms"][0]
print(json.dumps(res))
