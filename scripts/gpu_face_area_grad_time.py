"""Time of radfoam.face_area_grad (the kernels of rf_face_area_grad.hip) next to radfoam.cell_geometry and
radfoam.cell_geometry_grad in the same run, on the cloud of DESIGN 4.7: 2 M points uniform in [-1,1]^3 (seed 0)
triangulated on the GPU.  HIP events around the whole Python call (kernels, bbox, status read-back), 3 warm-up calls,
median (min, max) of 5.  The upstreams are random; ``backward`` is forward plus backward through
differentiable_cell_geometry(face_area=True) of a loss on the finite face areas alone.

    python scripts/gpu_face_area_grad_time.py [--points 2000000]      # prints one JSON line
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
g = torch.Generator(device=dev).manual_seed(1)
gv = torch.rand(N, dtype=torch.float64, device=dev, generator=g) * 2 - 1
gc = torch.rand((N, 3), dtype=torch.float64, device=dev, generator=g) * 2 - 1
ga = torch.rand(E, dtype=torch.float64, device=dev, generator=g) * 2 - 1
grad = radfoam.face_area_grad(p, adj, off, geo, ga)
assert bool(torch.isfinite(grad).all())
fin = torch.isfinite(geo.face_area)


def forward_backward():
    q = p.clone().requires_grad_(True)
    out = radfoam.differentiable_cell_geometry(q, adj, off, face_area=True)
    out.face_area[fin].sum().backward()


res = {"points": N, "edges": E, "longest_row": int(rows.max()), "finite_faces": int(fin.sum()),
       "cell_geometry_ms": timed(lambda: radfoam.cell_geometry(p, adj, off)),
       "cell_geometry_grad_ms": timed(lambda: radfoam.cell_geometry_grad(p, adj, off, geo, gv, gc)),
       "face_area_grad_ms": timed(lambda: radfoam.face_area_grad(p, adj, off, geo, ga)),
       "differentiable_forward_backward_ms": timed(forward_backward)}
print(json.dumps(res))
