"""Regularising a foam whose sites move: Adam on the centroidal (Lloyd) energy plus an equal-volume penalty,

    loss = mean over bounded cells of |p_a - c_a|^2 / h^2  +  lambda * var(log V_a),      h = N^(-1/3),

through ``radfoam.differentiable_cell_geometry``.  The triangulation is rebuilt on the GPU every step; the gradient
reaches the sites through the cells' volumes and centroids (and directly through p_a).  Unbounded cells (the hull) have
volume +inf and centroid NaN and are masked out of the loss.

    python examples/foam_lloyd.py [--points 4000] [--steps 50] [--lam 0.1]
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import radfoam  # noqa: E402
from radfoam_amd.triangulation import Triangulation  # noqa: E402


def lloyd_loss(points, geo, lam):
    b = geo.bounded
    h = float(points.size(0)) ** (-1.0 / 3.0)
    spread = ((points[b].double() - geo.centroid[b]) ** 2).sum(1).mean() / (h * h)
    return spread + lam * torch.log(geo.volume[b]).var()


def run(num_points=4000, steps=50, lam=0.1, lr=2e-3, seed=0, device="cuda:0", quiet=False):
    """The loss before every step and after the last one (steps + 1 numbers)."""
    dev = torch.device(device)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    start = (torch.rand((num_points, 3), generator=gen) * 2.0 - 1.0).to(dev)
    tri = Triangulation(start)
    points = start[tri.permutation().to(torch.int64)].clone().requires_grad_(True)      # kd-order, kept from here on
    opt = torch.optim.Adam([points], lr=lr)
    losses = []
    for step in range(steps + 1):
        if step:
            tri.rebuild(points, incremental=True)
        geo = radfoam.differentiable_cell_geometry(points, tri.point_adjacency(), tri.point_adjacency_offsets())
        loss = lloyd_loss(points, geo, lam)
        losses.append(float(loss.detach()))
        if not quiet:
            print(f"step {step:3d}: loss {losses[-1]:.6f} over {int(geo.bounded.sum())} bounded cells")
        if step == steps:
            break
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    return losses


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--lam", type=float, default=0.1)
    ap.add_argument("--lr", type=float, default=2e-3)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    run(args.points, args.steps, args.lam, args.lr, args.seed)


if __name__ == "__main__":
    main()
