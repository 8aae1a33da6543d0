"""The level set of a foam's density as a smooth mesh, and a loss on its vertices: ``radfoam.isosurface`` runs marching
tetrahedra over the Delaunay tetrahedra of the sites (``Triangulation.tets()``), every vertex on a Delaunay edge where the
density interpolated between its two sites crosses the level.  The mesh is written as an indexed PLY, with a per-site
colour carried to the vertices by ``vertex_t``, and Adam pulls the vertices onto a sphere,

    loss = mean over the mesh's vertices of (|v - c| - r)^2,

through ``mesh.vertices``, which carries autograd to the sites and to the densities.  The topology is extracted again every
step: the triangulation is rebuilt incrementally, ``Triangulation.tets()`` reads the tetrahedra back off the new neighbour
lists on the GPU (``radfoam.delaunay_tets``) and ``radfoam.isosurface`` runs over them.  With ``--every K`` only every
K-th step does; in between ``radfoam.isosurface_vertices`` re-evaluates the vertices of the last topology, which costs one
kernel and no triangulation.  The wall time of every step is printed.

    python examples/foam_isosurface.py [--points 4000] [--steps 40] [--every 1] [--ply surface.ply]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import radfoam  # noqa: E402
from radfoam_amd.triangulation import Triangulation  # noqa: E402


def vertex_colours(mesh, colours):
    """a per-site attribute [N,C] at the vertices: the same interpolation along a -> b that placed them"""
    a, b = mesh.vertex_sites[:, 0], mesh.vertex_sites[:, 1]
    return torch.lerp(colours[a].to(torch.float64), colours[b].to(torch.float64), mesh.vertex_t[:, None])


def write_ply(path, mesh, colours=None):
    """the triangles of an IsoMesh over its welded vertices, as an ASCII PLY; ``colours`` f[V,3] in [0,1]"""
    v = mesh.vertices.detach().cpu().numpy()
    tri = mesh.triangles.cpu().numpy()
    with open(path, "w") as f:
        f.write(f"ply\nformat ascii 1.0\nelement vertex {len(v)}\nproperty double x\nproperty double y\nproperty double z\n")
        if colours is not None:
            f.write("property uchar red\nproperty uchar green\nproperty uchar blue\n")
        f.write(f"element face {len(tri)}\nproperty list uchar int vertex_indices\nend_header\n")
        if colours is None:
            np.savetxt(f, v, fmt="%.17g")
        else:
            rgb = (colours.detach().clamp(0, 1) * 255).round().cpu().numpy().astype(np.int64)
            for x, c in zip(v, rgb):
                f.write(f"{x[0]:.17g} {x[1]:.17g} {x[2]:.17g} {c[0]} {c[1]} {c[2]}\n")
        np.savetxt(f, np.concatenate([np.full((len(tri), 1), 3), tri], 1), fmt="%d")


def sphere_loss(vertices, centre, radius):
    return (((vertices - centre).norm(dim=1) - radius) ** 2).mean()


def run(num_points=4000, steps=40, every=1, lr=2e-3, radius=0.6, level=0.5, seed=0, device="cuda:0", quiet=False,
        ply=None):
    """(loss, vertices, triangles, extracted, seconds) before every step and after the last one (steps + 1 tuples;
    seconds: the wall time of the step, its extraction, loss, backward and update).  The density starts as a bumpy ball,
    1 at the centre and falling through ``level`` near |p| = ``radius``."""
    dev = torch.device(device)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    start = (torch.rand((num_points, 3), generator=gen) * 2.0 - 1.0).to(dev)
    tri = Triangulation(start)
    points = start[tri.permutation().to(torch.int64)].clone()                           # kd-order, kept from here on
    r = points.norm(dim=1)
    bumps = 0.08 * torch.sin(7.0 * points[:, 0]) * torch.cos(5.0 * points[:, 1])
    density = (1.0 - (1.0 - level) * r / radius + bumps).to(torch.float32)
    colours = 0.5 + 0.5 * points / points.abs().max()                                   # a per-site attribute to carry along
    points.requires_grad_(True), density.requires_grad_(True)
    centre = torch.zeros(3, dtype=torch.float64, device=dev)
    opt = torch.optim.Adam([points, density], lr=lr)
    history, sites = [], None
    for step in range(steps + 1):
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        began = time.perf_counter()
        extract = step % every == 0 or step == steps
        if extract:
            if step:
                tri.rebuild(points, incremental=True)
            mesh = radfoam.isosurface(points, tri.tets(), density, level)
            vertices, sites, triangles = mesh.vertices, mesh.vertex_sites, mesh.triangles.size(0)
        else:
            vertices = radfoam.isosurface_vertices(points, density, sites, level)       # the last topology, moved along
        loss = sphere_loss(vertices, centre, radius)
        if step < steps:
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        history.append((float(loss.detach()), vertices.size(0), triangles, extract, time.perf_counter() - began))
        if not quiet:
            print(f"step {step:3d}: loss {history[-1][0]:.6e}  vertices {history[-1][1]}  triangles {triangles}"
                  f"  {1e3 * history[-1][4]:.2f} ms" + ("  (extracted)" if extract else ""))
        if step == steps and ply:
            write_ply(ply, mesh, vertex_colours(mesh, colours))
    return history


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--every", type=int, default=1, help="extract the topology again every this many steps")
    ap.add_argument("--lr", type=float, default=2e-3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--ply", default=None, help="write the final mesh here")
    a = ap.parse_args()
    history = run(a.points, a.steps, a.every, a.lr, seed=a.seed, ply=a.ply)
    extracting = sorted(h[4] for h in history[1:] if h[3])
    print(f"sphere loss {history[0][0]:.6e} -> {history[-1][0]:.6e}; a step that extracts the topology: median "
          f"{1e3 * extracting[len(extracting) // 2]:.2f} ms")


if __name__ == "__main__":
    main()
