"""Time of radfoam.cell_moments_in_box (the kernels of rf_cell_box_moments.hip) next to radfoam.cell_geometry_in_box and
radfoam.cell_moments in the same run, on the cloud of DESIGN 4.7: 2 M points uniform in [-1,1]^3 (seed 0) triangulated on
the GPU, in the box [-1,1]^3.  HIP events around the whole Python call (kernels, bbox, status read-back), 3 warm-up calls,
median (min, max) of 5.  There is no earlier implementation to compare with: the figure to read is the ratio to
cell_geometry_in_box, which clips the same faces of the same lists and sums four numbers a face where this sums six.
Also the example's numbers on 4,000 points: the Gaussians written with and without the box, and the CVT energy sum tr
site_moment over all sites next to the bounded-only value.

    python scripts/gpu_cell_box_moments_time.py [--points 2000000]      # prints one JSON line
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import radfoam
from examples import foam_to_gaussians
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


mo = radfoam.cell_moments_in_box(p, adj, off, BOX)
geo = mo.geometry
assert bool(geo.nonempty.all()) and bool(torch.isfinite(mo.site_moment).all()) and bool(torch.isfinite(mo.central_moment).all())
e = torch.tensor([2.0, 2.0, 2.0], dtype=torch.float64, device=dev)
q = p.double()                                       # the box's centre is the origin
m = geo.centroid - q
diag = (mo.site_moment[:, :3] + geo.volume[:, None] * (2.0 * m * q + q * q)).sum(0)

res = {"points": N, "edges": E, "longest_row": int(rows.max()),
       "partition_diagonal_over_box": (diag / (8.0 * e * e / 12.0)).tolist(),
       "cell_geometry_in_box_ms": timed(lambda: radfoam.cell_geometry_in_box(p, adj, off, BOX)),
       "cell_moments_in_box_given_geometry_ms": timed(lambda: radfoam.cell_moments_in_box(p, adj, off, BOX, geometry=geo)),
       "cell_moments_in_box_ms": timed(lambda: radfoam.cell_moments_in_box(p, adj, off, BOX)),
       "cell_moments_ms": timed(lambda: radfoam.cell_moments(p, adj, off))}
base = res["cell_geometry_in_box_ms"][0]
res["ratio_to_cell_geometry_in_box"] = {k[:-3]: res[k][0] / base for k in res if k.endswith("_ms")}
del mo, geo, q, m, p, adj, off, tri, pts
with tempfile.TemporaryDirectory() as tmp:
    boxed = foam_to_gaussians.run(4000, os.path.join(tmp, "boxed.ply"), device=dev, quiet=True, box=BOX)
    plain = foam_to_gaussians.run(4000, os.path.join(tmp, "plain.ply"), device=dev, quiet=True)
res["example_4000"] = {"gaussians_with_box": boxed[0], "gaussians_without": plain[0], "cvt_energy_all_sites": boxed[1],
                       "cvt_energy_bounded_only": plain[1]}
print(json.dumps(res))
