"""Time of radfoam.cell_mesh (the kernels of rf_cell_mesh.hip and the welding in torch) next to radfoam.cell_surface in
the same run, on the cloud and selection of DESIGN 4.7: 2 M points uniform in [-1,1]^3 (seed 0) triangulated on the GPU,
``inside`` = a uniform random density (seed 1) above its median, within radius 0.8.  HIP events around the Python calls,
3 warm-up calls, median (min, max) of 5.  cell_mesh is also timed stage by stage (its own internal steps, called in its
order): the geometry, the emit (count, compaction, the two emit kernels, the status read-back), the weld (torch.unique
over the packed keys and the lowest corner per key), the vertex pick with the fans; then mesh_vertices, and forward plus
backward of the sphere loss through mesh.vertices.  ``surface_emit_ms`` is cell_surface minus cell_geometry, the stage the
emit replaces.

    python scripts/gpu_cell_mesh_time.py [--points 2000000]      # prints one JSON line
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import radfoam
from radfoam_amd import geometry as G
from radfoam_amd import mesh as M
from radfoam_amd.triangulation import Triangulation

N = int(sys.argv[sys.argv.index("--points") + 1]) if "--points" in sys.argv else 2000000
dev = "cuda:0"
gen = torch.Generator(device="cpu").manual_seed(0)
pts = (torch.rand((N, 3), generator=gen) * 2.0 - 1.0).to(dev)
tri = Triangulation(pts)
p = pts[tri.permutation().to(torch.int64)].contiguous()
adj, off = tri.point_adjacency(), tri.point_adjacency_offsets()
E = int(adj.numel())
density = torch.rand(N, generator=torch.Generator(device="cpu").manual_seed(1)).to(dev)
inside = (density > density.median()) & (p.norm(dim=1) < 0.8)
print("triangulated", N, E, int(inside.sum()), flush=True)


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


prep = G._prepare(p, adj, off)
geo, face_vertices = G._run_geometry(*prep)
slots, offsets, corner_xyz, corner_sites = M._emit(*prep, face_vertices, inside)
vertex_sites, polygon_vertices, first = M._weld(corner_sites)
mesh = radfoam.cell_mesh(p, adj, off, inside)
triangles, edge = radfoam.cell_surface(p, adj, off, inside)
assert torch.equal(mesh.triangle_slot, edge) and torch.equal(mesh.vertex_sites, vertex_sites)
T, C, V, F = int(edge.numel()), int(polygon_vertices.numel()), int(vertex_sites.size(0)), int(slots.numel())
worst = float((mesh.vertices[mesh.triangles] - triangles).abs().max())
centre = torch.zeros(3, dtype=torch.float64, device=dev)
del triangles, edge


def pick():
    corner_xyz[first]
    M._fans(offsets, polygon_vertices, slots)


def forward_backward():
    q = p.clone().requires_grad_(True)
    v = radfoam.cell_mesh(q, adj, off, inside).vertices
    (((v - centre).norm(dim=1) - 0.8) ** 2).mean().backward()


def backward_alone():
    q = p.clone().requires_grad_(True)
    v = radfoam.mesh_vertices(q, vertex_sites)
    (((v - centre).norm(dim=1) - 0.8) ** 2).mean().backward()


mesh_bytes = sum(int(t.numel()) * t.element_size() for t in mesh)
res = {"points": N, "edges": E, "inside": int(inside.sum()), "faces": F, "triangles": T, "corners": C, "vertices": V,
       "largest_polygon": int((offsets[1:] - offsets[:-1]).max()), "max_abs_vertex_minus_cell_surface": worst,
       "mesh_bytes": mesh_bytes, "mesh_bytes_without_triangles": mesh_bytes - 32 * T, "unwelded_bytes": 72 * T,
       "cell_geometry_ms": timed(lambda: G._run_geometry(*prep)),
       "cell_surface_ms": timed(lambda: radfoam.cell_surface(p, adj, off, inside)),
       "cell_mesh_ms": timed(lambda: radfoam.cell_mesh(p, adj, off, inside)),
       "emit_ms": timed(lambda: M._emit(*prep, face_vertices, inside)),
       "weld_ms": timed(lambda: M._weld(corner_sites)),
       "pick_and_fans_ms": timed(pick),
       "mesh_vertices_ms": timed(lambda: radfoam.mesh_vertices(p, vertex_sites)),
       "mesh_vertices_forward_backward_ms": timed(backward_alone),
       "cell_mesh_sphere_loss_forward_backward_ms": timed(forward_backward)}
res["surface_emit_ms"] = res["cell_surface_ms"][0] - res["cell_geometry_ms"][0]
print(json.dumps(res))
