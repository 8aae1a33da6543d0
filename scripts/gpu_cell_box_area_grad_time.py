"""Time of radfoam.face_area_in_box_grad (the kernels of rf_cell_box_area_grad.hip) next to radfoam.cell_geometry_in_box,
radfoam.cell_geometry_in_box_grad and radfoam.face_area_grad in the same run, on the cloud of DESIGN 4.7: 2 M points
uniform in [-1,1]^3 (seed 0) triangulated on the GPU, in the box [-1,1]^3.  HIP events around the whole Python call
(kernels, bbox, upstream conversion, status read-back), 3 warm-up calls, median (min, max) of 5.  There is no bar.
``handed_on_rows`` is the number of rows the lane-per-face kernel leaves to the serial one (rows over 64, row polygons over
16 vertices; the final polygons bound it from below).  ``sites_reached`` counts the sites with a nonzero gradient from
the same face upstream (plus a wall upstream in the box) through the boxed and through the unboxed operator.

    timeout -k 10 900 python scripts/gpu_cell_box_area_grad_time.py [--points 2000000]      # prints one JSON line
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
row_of = torch.repeat_interleave(torch.arange(N, device=dev), rows)
peak = torch.zeros(N, dtype=torch.int32, device=dev)
peak.scatter_reduce_(0, row_of, face_vertices, "amax")
handed = (rows > 64) | (peak > 16)
plain = radfoam.cell_geometry(p, adj, off)

g = torch.Generator(device="cpu").manual_seed(1)
size = geo.volume.pow(1.0 / 3.0)
ga = ((torch.rand(E, generator=g, dtype=torch.float64) * 2.0 - 1.0).to(dev) / size[row_of]).contiguous()
gw = ((torch.rand((N, 6), generator=g, dtype=torch.float64) * 2.0 - 1.0).to(dev) / size[:, None]).contiguous()
w = ((torch.rand(N, generator=g, dtype=torch.float64) * 2.0 - 1.0).to(dev) / size ** 2).contiguous()
u = (torch.rand((N, 3), generator=g, dtype=torch.float64) * 2.0 - 1.0).to(dev)
grad = radfoam.face_area_in_box_grad(p, adj, off, BOX, geo, ga, gw)
assert bool(torch.isfinite(grad).all())
unboxed = radfoam.face_area_grad(p, adj, off, plain, ga)
columns = torch.tensor([0.75, -0.5, 1.25, 0.375, -1.125, 0.875], dtype=torch.float64, device=dev).expand(N, 6).contiguous()
zero = radfoam.face_area_in_box_grad(p, adj, off, BOX, geo, None, columns)
q = p.clone().requires_grad_(True)


def through_the_wrapper():
    q.grad = None
    d = radfoam.differentiable_cell_geometry_in_box(q, adj, off, BOX, face_area=True)
    ((ga * d.face_area).sum() + (gw * d.wall_area).sum()).backward()


res = {"points": N, "edges": E, "longest_row": int(rows.max()),
       "handed_on_rows": int(handed.sum()),
       "largest_row_norm": float(grad.norm(dim=1).max()),
       "constant_wall_upstream_max_abs": float(zero.abs().max()),
       "sites_reached": {"face_area_in_box_grad": int((grad != 0).any(1).sum()),
                         "face_area_in_box_grad_faces_only": int(
                             (radfoam.face_area_in_box_grad(p, adj, off, BOX, geo, ga, None) != 0).any(1).sum()),
                         "face_area_grad": int((unboxed != 0).any(1).sum())},
       "cell_geometry_in_box_ms": timed(lambda: radfoam.cell_geometry_in_box(p, adj, off, BOX)),
       "cell_geometry_in_box_grad_ms": timed(lambda: radfoam.cell_geometry_in_box_grad(p, adj, off, BOX, geo, w, u)),
       "face_area_grad_ms": timed(lambda: radfoam.face_area_grad(p, adj, off, plain, ga)),
       "face_area_in_box_grad_ms": timed(lambda: radfoam.face_area_in_box_grad(p, adj, off, BOX, geo, ga, gw)),
       "face_area_in_box_grad_faces_only_ms": timed(lambda: radfoam.face_area_in_box_grad(p, adj, off, BOX, geo, ga, None)),
       "forward_plus_backward_ms": timed(through_the_wrapper)}
res["ratio_to_face_area_grad"] = res["face_area_in_box_grad_ms"][0] / res["face_area_grad_ms"][0]
print(json.dumps(res))
