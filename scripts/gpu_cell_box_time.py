"""Time of radfoam.cell_geometry_in_box (the kernels of rf_cell_box.hip) next to radfoam.cell_geometry in the same run, on
the cloud of DESIGN 4.7: 2 M points uniform in [-1,1]^3 (seed 0) triangulated on the GPU, in the box [-1,1]^3.  HIP events
around the whole Python call (kernels, bbox, status read-back), 3 warm-up calls, median (min, max) of 5.  There is no
earlier implementation to compare with: the figure to read is the ratio to cell_geometry, which clips the same faces by
six planes fewer and has six lanes fewer per row.  ``handed_on_share`` is the share of cells the lane-per-face kernel
leaves to the serial one (rows over 58, polygons over 16 vertices).

    python scripts/gpu_cell_box_time.py [--points 2000000]      # prints one JSON line
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


geo, face_vertices, wall_vertices = geometry._run_geometry_in_box(*geometry._prepare(p, adj, off), list(BOX))
assert bool(torch.isfinite(geo.volume).all()) and bool(geo.nonempty.all())
peak = torch.zeros(N, dtype=torch.int32, device=dev)      # the final polygons bound the hand-on from below
peak.scatter_reduce_(0, torch.repeat_interleave(torch.arange(N, device=dev), rows), face_vertices, "amax")
peak = torch.maximum(peak, wall_vertices.max(1).values)
handed = (rows > 58) | (peak > 16)

res = {"points": N, "edges": E, "longest_row": int(rows.max()),
       "sum_volume_over_box": float(geo.volume.sum()) / 8.0,
       "cells_touching_a_wall": int((geo.wall_area > 0).any(1).sum()),
       "handed_on_share_at_least": float(handed.double().mean()),
       "cell_geometry_ms": timed(lambda: radfoam.cell_geometry(p, adj, off)),
       "cell_geometry_in_box_ms": timed(lambda: radfoam.cell_geometry_in_box(p, adj, off, BOX))}
res["ratio_to_cell_geometry"] = res["cell_geometry_in_box_ms"][0] / res["cell_geometry_ms"][0]
print(json.dumps(res))
