"""Fit the Delaunay field of a foam to a signed distance at 3-D samples: ``Triangulation.locate`` finds the tetrahedron of
every sample, ``radfoam.interpolate`` evaluates the per-site ``values`` there (linear over every tetrahedron: the field
``radfoam.isosurface`` extracts the level set of), and Adam pulls

    loss = mean over the samples of (f(x_k) - (r - |x_k - c|))^2

down through ``FieldSamples.value``, which carries autograd to ``values`` and, with ``--move-points``, to the sites (then
the triangulation is rebuilt incrementally and the samples are located again every step).  Half of the samples lie on
the sphere |x - c| = r, half anywhere in the cube [-1,1]^3; samples outside the hull of the sites have no field and are
left out.  Before and after, the zero isosurface is extracted and the worst and the mean distance of its vertices
from the sphere are printed (a site no sample reaches keeps its start value, and the worst distance with it).  ``--grid n`` writes the fitted field on an n^3 grid over [-1,1]^3 to an .npy file (NaN outside the
hull).

    python examples/foam_field_samples.py [--points 4000] [--samples 40000] [--steps 200] [--move-points] [--grid 64]
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


def sphere_samples(count, radius, gen, dev):
    """float32 [count,3]: half of the samples on the sphere, half uniform in the cube [-1,1]^3, so that every site's value
    is supervised through some tetrahedron"""
    direction = torch.randn((count // 2, 3), generator=gen)
    on_sphere = radius * direction / direction.norm(dim=1, keepdim=True)
    around = torch.rand((count - count // 2, 3), generator=gen) * 2.0 - 1.0
    return torch.cat([on_sphere, around]).to(torch.float32).to(dev)


def surface_error(points, tri, values, radius):
    """the worst and the mean distance of the zero isosurface's vertices from the sphere, and their number"""
    mesh = radfoam.isosurface(points.detach(), tri.tets(), values.detach(), 0.0)
    if mesh.vertices.size(0) == 0:
        return float("nan"), float("nan"), 0
    distance = (mesh.vertices.norm(dim=1) - radius).abs()
    return float(distance.max()), float(distance.mean()), mesh.vertices.size(0)


def field_on_grid(points, tri, values, n):
    axis = torch.linspace(-1, 1, n, dtype=torch.float32, device=points.device)
    grid = torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), -1).contiguous()
    where = tri.locate(grid)
    return radfoam.interpolate(points.detach(), tri.tets(), values.detach(), grid, where.tet).value


def run(num_points=4000, num_samples=40000, steps=200, lr=2e-2, radius=0.6, move_points=False, seed=0, device="cuda:0",
        quiet=False, grid=0, out="field.npy"):
    """(surface error before, surface error after, losses): the worst and mean distance of the isosurface's vertices from
    the sphere and their number, before and after the fit, and the loss of every step"""
    dev = torch.device(device)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    start = (torch.rand((num_points, 3), generator=gen) * 2.0 - 1.0).to(dev)
    tri = Triangulation(start)
    points = start[tri.permutation().to(torch.int64)].clone()                           # kd-order, kept from here on
    values = (0.3 * torch.randn(num_points, generator=gen)).to(dev) + (0.5 - points.norm(dim=1))   # a noisy, wrong ball
    samples = sphere_samples(num_samples, radius, gen, dev)
    target = (radius - samples.norm(dim=1)).to(torch.float64)
    values.requires_grad_(True)
    params = [values]
    if move_points:
        points.requires_grad_(True)
        params.append(points)
    opt = torch.optim.Adam(params, lr=lr)
    before = surface_error(points, tri, values, radius)
    where, losses = tri.locate(samples), []
    for step in range(steps):
        if move_points and step:
            tri.rebuild(points.detach(), incremental=True)
            where = tri.locate(samples)
        inside = where.tet >= 0                                                          # samples outside the hull: no field
        field = radfoam.interpolate(points, tri.tets(), values, samples, where.tet).value
        loss = ((field[inside] - target[inside]) ** 2).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        if not quiet and (step % 20 == 0 or step == steps - 1):
            print(f"step {step:4d}: loss {losses[-1]:.6e}  located {int(inside.sum())} of {num_samples}, "
                  f"at most {int(where.hops.max())} hops")
    if move_points and steps:
        tri.rebuild(points.detach(), incremental=True)
    after = surface_error(points, tri, values, radius)
    if grid:
        np.save(out, field_on_grid(points, tri, values, grid).cpu().numpy())
    return before, after, losses


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--samples", type=int, default=40000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--lr", type=float, default=2e-2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--move-points", action="store_true", help="fit the sites too; rebuild and locate again every step")
    ap.add_argument("--grid", type=int, default=0, help="write the fitted field on an n^3 grid to --out")
    ap.add_argument("--out", default="field.npy")
    a = ap.parse_args()
    before, after, losses = run(a.points, a.samples, a.steps, a.lr, move_points=a.move_points, seed=a.seed, grid=a.grid, out=a.out)
    print(f"loss {losses[0]:.6e} -> {losses[-1]:.6e}; isosurface vertices' worst distance from the sphere: "
          f"{before[0]:.4f} (mean {before[1]:.4f}, {before[2]} vertices) -> {after[0]:.4f} (mean {after[1]:.4f}, {after[2]} "
          "vertices)")


if __name__ == "__main__":
    main()
