"""The foam's own surface as a mesh, and a loss on its vertices: ``radfoam.cell_mesh`` welds the faces between ``inside``
and ``outside`` cells into polygons over shared vertices (written here as an indexed PLY), and Adam pulls those vertices
onto a sphere,

    loss = mean over the mesh's vertices of (|v - c| - r)^2,

through ``mesh.vertices``, which carries autograd to the sites.  ``inside`` is fixed per site: the cells whose sites start
within a ball.  The triangulation is rebuilt on the GPU every step, and with it the mesh.

    python examples/foam_mesh.py [--points 4000] [--steps 50] [--ply surface.ply]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import radfoam  # noqa: E402
from radfoam_amd.triangulation import Triangulation  # noqa: E402


def write_ply(path, mesh):
    """the polygons of a CellMesh over its welded vertices, as an ASCII PLY"""
    v = mesh.vertices.detach().cpu().numpy()
    off, pv = mesh.polygon_offsets.cpu().numpy(), mesh.polygon_vertices.cpu().numpy()
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\n"
                f"element vertex {len(v)}\nproperty double x\nproperty double y\nproperty double z\n"
                f"element face {len(off) - 1}\nproperty list uchar int vertex_indices\nend_header\n")
        np.savetxt(f, v, fmt="%.17g")
        for i in range(len(off) - 1):
            ring = pv[off[i]:off[i + 1]]
            f.write(f"{len(ring)} " + " ".join(map(str, ring)) + "\n")


def sphere_loss(vertices, centre, radius):
    return (((vertices - centre).norm(dim=1) - radius) ** 2).mean()


def run(num_points=4000, steps=50, lr=1e-3, radius=0.6, seed=0, device="cuda:0", quiet=False, start=None, ply=None):
    """(loss, vertices, polygons) before every step and after the last one (steps + 1 triples).  ``start``: the sites as
    a float32 [N,3] array instead of ``num_points`` uniform ones."""
    dev = torch.device(device)
    if start is None:
        gen = torch.Generator(device="cpu").manual_seed(seed)
        start = torch.rand((num_points, 3), generator=gen) * 2.0 - 1.0
    start = torch.as_tensor(start, dtype=torch.float32).to(dev)
    tri = Triangulation(start)
    points = start[tri.permutation().to(torch.int64)].clone().requires_grad_(True)      # kd-order, kept from here on
    inside = points.detach().norm(dim=1) < radius
    centre = torch.zeros(3, dtype=torch.float64, device=dev)
    opt = torch.optim.Adam([points], lr=lr)
    history = []
    for step in range(steps + 1):
        if step:
            tri.rebuild(points, incremental=True)
        mesh = radfoam.cell_mesh(points, tri.point_adjacency(), tri.point_adjacency_offsets(), inside)
        loss = sphere_loss(mesh.vertices, centre, radius)
        history.append((float(loss.detach()), mesh.vertices.size(0), mesh.polygon_slot.numel()))
        if not quiet:
            print(f"step {step:3d}: loss {history[-1][0]:.6e}  vertices {history[-1][1]}  polygons {history[-1][2]}")
        if step == steps:
            if ply:
                write_ply(ply, mesh)
            break
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    return history


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--ply", default=None, help="write the final mesh here")
    a = ap.parse_args()
    history = run(a.points, a.steps, a.lr, seed=a.seed, ply=a.ply)
    print(f"sphere loss {history[0][0]:.6e} -> {history[-1][0]:.6e}")


if __name__ == "__main__":
    main()
