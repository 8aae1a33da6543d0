"""Time of radfoam.cell_moments_in_box_grad (the kernels of rf_cell_box_moments_grad.hip) next to
radfoam.cell_geometry_in_box_grad in the same run, on the cloud of DESIGN 4.7: 2 M points uniform in [-1,1]^3 (seed 0)
triangulated on the GPU, in the box [-1,1]^3.  HIP events around the whole Python call (kernels, bbox, upstream conversion,
status read-back), 3 warm-up calls, median (min, max) of 5.  Rows: cell_geometry_in_box_grad; the new operator with the
moment upstreams only; with all four upstreams (the fused call); the two-launch alternative (the new operator for the
moments plus cell_geometry_in_box_grad, added); forward plus .backward() of a loss of all four outputs through
differentiable_cell_moments_in_box.  There is no bar.  ``handed_on_share_at_least`` is the share of rows the lane-per-face
kernel leaves to the serial one (rows over 64, row polygons over 16 vertices; the final polygons bound it from below);
``cvt_closed_form_worst`` is check (a) on the whole cloud, |grad - 2 V (p - c)| over V max(longest |d|, |c - p|) per row.
With ``--example`` it also runs examples/foam_cvt_box.py with the CVT energy on 4,000 points.

    timeout -k 10 900 python scripts/gpu_cell_box_moments_grad_time.py [--points 2000000] [--example]   # one JSON line
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

g = torch.Generator(device="cpu").manual_seed(1)
size = geo.volume.pow(1.0 / 3.0)
rand = lambda *shape: (torch.rand(shape, generator=g, dtype=torch.float64) * 2.0 - 1.0).to(dev)
gq = (rand(N, 6) / size[:, None] ** 4).contiguous()
gm = (rand(N, 6) / size[:, None] ** 4).contiguous()
w = (rand(N) / size ** 2).contiguous()
u = rand(N, 3)
grad = radfoam.cell_moments_in_box_grad(p, adj, off, BOX, geo, gq, gm, w, u)
assert bool(torch.isfinite(grad).all())
halves = radfoam.cell_moments_in_box_grad(p, adj, off, BOX, geo, gq, gm) + radfoam.cell_geometry_in_box_grad(
    p, adj, off, BOX, geo, w, u)

# check (a) on the whole cloud
trace = torch.tensor([1.0, 1.0, 1.0, 0.0, 0.0, 0.0], dtype=torch.float64, device=dev).expand(N, 6).contiguous()
cvt = radfoam.cell_moments_in_box_grad(p, adj, off, BOX, geo, trace)
m = geo.centroid - p.double()
longest = torch.zeros(N, dtype=torch.float64, device=dev)
longest.scatter_reduce_(0, row_of, (p[adj.to(torch.int64)].double() - p[row_of].double()).norm(dim=1), "amax")
scale = geo.volume * torch.maximum(longest, m.norm(dim=1))
closed = ((cvt + 2.0 * geo.volume[:, None] * m).norm(dim=1) / scale).max()

q = p.clone().requires_grad_(True)


def through_the_wrapper():
    q.grad = None
    d = radfoam.differentiable_cell_moments_in_box(q, adj, off, BOX)
    ((gq * d.site_moment).sum() + (gm * d.central_moment).sum() + (w * d.geometry.volume).sum()
     + (u * d.geometry.centroid).sum()).backward()


def two_launches():
    return radfoam.cell_moments_in_box_grad(p, adj, off, BOX, geo, gq, gm) + radfoam.cell_geometry_in_box_grad(
        p, adj, off, BOX, geo, w, u)


res = {"points": N, "edges": E, "longest_row": int(rows.max()),
       "handed_on_share_at_least": float(handed.double().mean()), "handed_on_rows_at_least": int(handed.sum()),
       "largest_row_norm": float(grad.norm(dim=1).max()),
       "fused_against_two_launches_worst": float(((grad - halves).norm(dim=1) / halves.norm(dim=1).clamp(min=1.0)).max()),
       "cvt_closed_form_worst": float(closed), "cvt_energy": float(radfoam.cell_moments_in_box(
           p, adj, off, BOX, geo).site_moment[:, :3].sum()),
       "cell_geometry_in_box_grad_ms": timed(lambda: radfoam.cell_geometry_in_box_grad(p, adj, off, BOX, geo, w, u)),
       "cell_moments_in_box_grad_moments_only_ms": timed(
           lambda: radfoam.cell_moments_in_box_grad(p, adj, off, BOX, geo, gq, gm)),
       "cell_moments_in_box_grad_all_four_ms": timed(
           lambda: radfoam.cell_moments_in_box_grad(p, adj, off, BOX, geo, gq, gm, w, u)),
       "two_launches_ms": timed(two_launches),
       "forward_plus_backward_ms": timed(through_the_wrapper)}
res["ratio_to_cell_geometry_in_box_grad"] = (res["cell_moments_in_box_grad_all_four_ms"][0]
                                             / res["cell_geometry_in_box_grad_ms"][0])
res["fused_saves_ms"] = res["two_launches_ms"][0] - res["cell_moments_in_box_grad_all_four_ms"][0]

if "--example" in sys.argv:
    from examples import foam_cvt_box

    del grad, halves, cvt, gq, gm, w, u, q
    for name, kwargs in (("cvt", dict(energy="cvt")), ("cvt_equal_volume_aniso", dict(energy="cvt", equal_volume=1.0,
                                                                                       aniso=0.1))):
        got = foam_cvt_box.run(num_points=4000, steps=8, device=dev, quiet=True, **kwargs)
        res["example_" + name] = {"energy_first": got[0][1], "energy_last": got[-1][1],
                                  "all_gradients_finite": all(r[2] for r in got),
                                  "worst_sum_v_over_v_box_minus_1": max(abs(r[0] - 1.0) for r in got)}
print(json.dumps(res))
