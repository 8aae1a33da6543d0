"""A voxel grid of a foam's own density: the field the tracer renders is piecewise constant on the Voronoi cells, so the
density (and colour) at a point are those of the site nearest to it.  ``Triangulation.locate_cells`` finds that site for
every voxel centre of an n^3 grid over [-1,1]^3 by the exact greedy walk over the neighbour lists, and ``density[cell]``
(with ``--rgb`` the DC colour too, four channels) is written as an .npy volume.

The foam is synthetic: sites uniform in the cube, density an analytic blob (a Gaussian around ``--centre`` cut to zero below
``--threshold``), colour the site's position mapped to [0,1].  Printed: the share of occupied voxels (density > 0), the hop
statistics of the walks, and with ``--check`` the number of voxels of the middle slice whose cell differs from
``nearest_point`` (the brute-force fp32 operator; a difference needs two sites whose fp32 distances round alike).

    python examples/foam_density_grid.py [--points 4000] [--grid 64] [--rgb] [--check] [--out density.npy]
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

from radfoam_amd.scene_ops import nearest_point  # noqa: E402
from radfoam_amd.triangulation import Triangulation  # noqa: E402


def blob_density(points, centre, width, threshold, peak=20.0):
    """float32 [N]: peak * exp(-|x - c|^2 / (2 width^2)), zero below ``threshold``"""
    r2 = ((points - torch.tensor(centre, dtype=points.dtype, device=points.device)) ** 2).sum(1)
    density = peak * torch.exp(-r2 / (2.0 * width * width))
    return torch.where(density >= threshold, density, torch.zeros_like(density))


def voxel_centres(n, dev):
    axis = (torch.arange(n, dtype=torch.float32, device=dev) + 0.5) * (2.0 / n) - 1.0
    return torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), -1).contiguous()


def run(num_points=4000, grid=64, rgb=False, check=False, centre=(0.1, -0.2, 0.0), width=0.35, threshold=1.0, seed=0,
        device="cuda:0", out=None, quiet=False):
    """dict(volume f32[n,n,n] or [n,n,n,4], occupied share, mean and largest hop count, differing voxels of the checked
    slice or None)"""
    dev = torch.device(device)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    raw = (torch.rand((num_points, 3), generator=gen) * 2.0 - 1.0).to(dev)
    tri = Triangulation(raw)
    points = raw[tri.permutation().to(torch.int64)].contiguous()                        # kd-order: the object's own
    density = blob_density(points, centre, width, threshold)
    centres = voxel_centres(grid, dev)
    where = tri.locate_cells(centres)
    volume = density[where.cell]
    if rgb:
        volume = torch.cat([volume[..., None], (0.5 * (points + 1.0))[where.cell]], -1)
    hops = where.hops.to(torch.float64)
    res = dict(volume=volume.cpu().numpy(), occupied=float((density[where.cell] > 0).double().mean()),
               hops_mean=float(hops.mean()), hops_max=int(hops.max()), differ=None)
    if check:
        middle = centres[grid // 2]
        brute = nearest_point(points, middle).view(torch.int32).to(torch.int64)
        res["differ"] = int((brute != where.cell[grid // 2]).sum())
    if out:
        np.save(out, res["volume"])
    if not quiet:
        print(f"{num_points} sites, {grid}^3 voxels: {100 * res['occupied']:.2f} % occupied, {res['hops_mean']:.2f} hops a "
              f"voxel on average, at most {res['hops_max']}" + (f", wrote {out} {res['volume'].shape}" if out else ""))
        if check:
            print(f"middle slice against nearest_point: {res['differ']} of {grid * grid} voxels differ")
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--rgb", action="store_true", help="write the DC colour beside the density: a [n,n,n,4] volume")
    ap.add_argument("--check", action="store_true", help="compare the middle slice against nearest_point")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="density.npy")
    a = ap.parse_args()
    res = run(a.points, a.grid, a.rgb, a.check, seed=a.seed, out=a.out)
    if a.check and res["differ"]:
        sys.exit("the checked slice differs from nearest_point")


if __name__ == "__main__":
    main()
