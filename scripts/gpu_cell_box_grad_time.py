"""Time of radfoam.cell_geometry_in_box_grad (the kernels of rf_cell_box_grad.hip) next to radfoam.cell_geometry_in_box in
the same run, on the cloud of DESIGN 4.7: 2 M points uniform in [-1,1]^3 (seed 0) triangulated on the GPU, in the box
[-1,1]^3.  HIP events around the whole Python call (kernels, bbox, upstream conversion, status read-back), 3 warm-up
calls, median (min, max) of 5.  Rows: the forward; the gradient with both upstreams; with grad_centroid=None; forward
plus .backward() of sum w V + u . c through differentiable_cell_geometry_in_box.  There is no bar: the figure to read is
the ratio to the forward, which clips the same row faces by the same planes and six wall faces besides.
``handed_on_share_at_least`` is the share of rows the lane-per-face kernel leaves to the serial one (rows over 64, row
polygons over 16 vertices; the final polygons bound it from below).

    timeout -k 10 900 python scripts/gpu_cell_box_grad_time.py [--points 2000000]      # prints one JSON line
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import radfoam
from radfoam_amd import geometry
from radfoam_amd.triangulation import Triangulation

N = int(sys.argv[sys.argv.index("--points") + 1]) if "--points" in sys.argv else 2000000
BOX = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
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


geo, face_vertices, _ = geometry._run_geometry_in_box(*geometry._prepare(p, adj, off), list(BOX))
assert bool(torch.isfinite(geo.volume).all()) and bool(geo.nonempty.all())
peak = torch.zeros(N, dtype=torch.int32, device=dev)
peak.scatter_reduce_(0, torch.repeat_interleave(torch.arange(N, device=dev), rows), face_vertices, "amax")
handed = (rows > 64) | (peak > 16)

g = torch.Generator(device="cpu").manual_seed(1)
size = geo.volume.pow(1.0 / 3.0)
w = ((torch.rand(N, generator=g, dtype=torch.float64) * 2.0 - 1.0).to(dev) / size ** 2).contiguous()
u = (torch.rand((N, 3), generator=g, dtype=torch.float64) * 2.0 - 1.0).to(dev)
grad = radfoam.cell_geometry_in_box_grad(p, adj, off, BOX, geo, w, u)
assert bool(torch.isfinite(grad).all())
zero = radfoam.cell_geometry_in_box_grad(p, adj, off, BOX, geo, torch.ones_like(w), None)
q = p.clone().requires_grad_(True)


def through_the_wrapper():
    q.grad = None
    d = radfoam.differentiable_cell_geometry_in_box(q, adj, off, BOX)
    ((w * d.volume).sum() + (u * d.centroid).sum()).backward()


res = {"points": N, "edges": E, "longest_row": int(rows.max()),
       "handed_on_share_at_least": float(handed.double().mean()),
       "largest_row_norm": float(grad.norm(dim=1).max()),
       "constant_volume_upstream_max_abs": float(zero.abs().max()),
       "cell_geometry_in_box_ms": timed(lambda: radfoam.cell_geometry_in_box(p, adj, off, BOX)),
       "cell_geometry_in_box_grad_ms": timed(lambda: radfoam.cell_geometry_in_box_grad(p, adj, off, BOX, geo, w, u)),
       "cell_geometry_in_box_grad_volume_only_ms": timed(
           lambda: radfoam.cell_geometry_in_box_grad(p, adj, off, BOX, geo, w, None)),
       "forward_plus_backward_ms": timed(through_the_wrapper)}
res["ratio_to_cell_geometry_in_box"] = res["cell_geometry_in_box_grad_ms"][0] / res["cell_geometry_in_box_ms"][0]
print(json.dumps(res))
