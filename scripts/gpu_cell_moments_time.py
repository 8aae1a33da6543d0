"""Time of radfoam.cell_moments (the kernels of rf_cell_moments.hip) next to radfoam.cell_geometry in the same run, on
the cloud of DESIGN 4.7: 2 M points uniform in [-1,1]^3 (seed 0) triangulated on the GPU.  HIP events around the whole
Python call (kernels, bbox, status read-back), 3 warm-up calls, median (min, max) of 5.  ``cell_moments_ms`` is the
operator alone, given the geometry; ``cell_moments_with_geometry_ms`` lets it run cell_geometry first.  There is no
earlier implementation to compare with: the figure to read is the ratio to cell_geometry, which clips the same faces.

    python scripts/gpu_cell_moments_time.py [--points 2000000]      # prints one JSON line
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
mo = radfoam.cell_moments(p, adj, off, geo)
b = geo.bounded
assert bool(torch.isfinite(mo.site_moment[b]).all()) and bool(torch.isnan(mo.site_moment[~b]).all())

res = {"points": N, "edges": E, "longest_row": int(rows.max()), "bounded_cells": int(b.sum()),
       "cvt_energy": float(mo.site_moment[b][:, :3].sum()),
       "cell_geometry_ms": timed(lambda: radfoam.cell_geometry(p, adj, off)),
       "cell_moments_ms": timed(lambda: radfoam.cell_moments(p, adj, off, geo)),
       "cell_moments_with_geometry_ms": timed(lambda: radfoam.cell_moments(p, adj, off))}
res["ratio_to_cell_geometry"] = res["cell_moments_ms"][0] / res["cell_geometry_ms"][0]
print(json.dumps(res))
