"""Shrinking the foam's own surface while the sites move: Adam on the summed area of the faces between ``inside`` and
``outside`` cells (the surface ``radfoam.cell_surface`` extracts) under a volume penalty,

    loss = sum of A_ab over faces with inside[a] != inside[b]  /  A_0   +   mu * ((sum of V_a over inside) / V_0 - 1)^2,

A_0 and V_0 the surface and the volume at the start, through ``radfoam.differentiable_cell_geometry(..., face_area=True)``.
``inside`` is fixed per site: the cells whose sites start within a ball.  The triangulation is rebuilt on the GPU every
step; the gradient reaches the sites through the face areas (the staircase of cell faces is smoothed) and the volumes.

    python examples/foam_surface_area.py [--points 4000] [--steps 50] [--mu 10]
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


def surface_and_volume(geo, adj, off, inside):
    """(area of the faces that leave the inside cells, each face once; volume of the inside cells)"""
    rows = torch.repeat_interleave(torch.arange(inside.numel(), device=inside.device),
                                   off[1:].to(torch.int64) - off[:-1].to(torch.int64))
    out = inside[rows] & ~inside[adj.to(torch.int64)] & torch.isfinite(geo.face_area)
    return geo.face_area[out].sum(), geo.volume[inside].sum()


def run(num_points=4000, steps=50, mu=10.0, lr=1e-3, radius=0.6, seed=0, device="cuda:0", quiet=False):
    """(loss, surface area, inside volume) before every step and after the last one (steps + 1 triples)."""
    dev = torch.device(device)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    start = (torch.rand((num_points, 3), generator=gen) * 2.0 - 1.0).to(dev)
    tri = Triangulation(start)
    points = start[tri.permutation().to(torch.int64)].clone().requires_grad_(True)      # kd-order, kept from here on
    inside = points.detach().norm(dim=1) < radius
    opt = torch.optim.Adam([points], lr=lr)
    history, area0, volume0 = [], None, None
    for step in range(steps + 1):
        if step:
            tri.rebuild(points, incremental=True)
        adj, off = tri.point_adjacency(), tri.point_adjacency_offsets()
        geo = radfoam.differentiable_cell_geometry(points, adj, off, face_area=True)
        if not bool(geo.bounded[inside].all()):
            raise RuntimeError("an inside cell is unbounded: choose a smaller radius")
        area, volume = surface_and_volume(geo, adj, off, inside)
        if step == 0:
            area0, volume0 = float(area.detach()), float(volume.detach())
        loss = area / area0 + mu * (volume / volume0 - 1.0) ** 2
        history.append((float(loss.detach()), float(area.detach()), float(volume.detach())))
        if not quiet:
            print(f"step {step:3d}: loss {history[-1][0]:.6f}  surface {history[-1][1]:.6f}  volume {history[-1][2]:.6f}")
        if step == steps:
            break
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    return history


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--mu", type=float, default=10.0)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    history = run(a.points, a.steps, a.mu, a.lr, seed=a.seed)
    print(f"surface {history[0][1]:.6f} -> {history[-1][1]:.6f}, inside volume {history[0][2]:.6f} -> {history[-1][2]:.6f}")


if __name__ == "__main__":
    main()
