"""A shading model of one's own along the tracer's rays: ``Pipeline.trace_segments`` exports the walk of every ray once,
``radfoam.composite_segments`` composites it in torch, and autograd does the rest.  Here the colour of a cell is not a
spherical-harmonics row but three free numbers per cell behind a sigmoid, fitted with Adam to the picture the foam's own
SH-degree-0 colours give; the density stays the foam's.

    python examples/custom_shading.py [--points 20000] [--width 128] [--height 96] [--steps 30]
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
from radfoam_amd import foam  # noqa: E402


def fit(num_points=20000, width=128, height=96, steps=30, seed=0, lr=0.1, device="cuda:0", log=print):
    """Returns the loss (mean squared error over rgb) before the first and after the last step."""
    fm = foam.make_synthetic_foam(num_points, 0, seed)
    dev = torch.device(device)
    points, attributes = torch.from_numpy(fm["points"]).to(dev), torch.from_numpy(fm["attributes"]).to(dev)
    adjacency = torch.from_numpy(fm["point_adjacency"]).to(dev)
    offsets = torch.from_numpy(fm["point_adjacency_offsets"]).to(dev)
    cam = foam.default_camera(width, height)
    rays = torch.from_numpy(foam.camera_rays(cam)).to(dev)
    start = torch.full(rays.shape[:-1], foam.nearest_point(fm["points"], cam["position"]), dtype=torch.int64,
                       device=dev).to(torch.uint32)

    pipe = radfoam.create_pipeline(0)
    target = pipe.trace_forward(points, attributes, adjacency, offsets, rays, start)["rgba"].reshape(-1, 4)[:, :3]
    seg = pipe.trace_segments(points, attributes, adjacency, offsets, rays, start)     # once: the walk does not change
    log(f"{rays.numel() // 6} rays, {seg['cells'].numel()} entries, longest walk "
        f"{int((seg['offsets'][1:] - seg['offsets'][:-1]).max())} cells")

    density = attributes[:, -1].contiguous()
    logits = torch.zeros((num_points, 3), device=dev, requires_grad=True)
    opt = torch.optim.Adam([logits], lr=lr)
    first = last = None
    for step in range(steps):
        opt.zero_grad()
        rgba = radfoam.composite_segments(seg, density, torch.sigmoid(logits))
        loss = ((rgba[:, :3] - target) ** 2).mean()
        loss.backward()
        opt.step()
        last = float(loss.detach())
        first = last if first is None else first
        if step % 10 == 0 or step == steps - 1:
            log(f"step {step:3d}  mse {last:.6f}")
    return first, last


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--height", type=int, default=96)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    first, last = fit(args.points, args.width, args.height, args.steps, args.seed)
    print(f"mse {first:.6f} -> {last:.6f}")


if __name__ == "__main__":
    main()
